"""What a map view must hold, built from the doubles a download returns and the definition in include/gridmapslam.h ("map views") --
pure numpy, no device: GridMap.render's grey chain (J/slam/GridMap.java:371-388, J/app/Util.java:92-107), the library's clamp and
its decimation rule.  Shared by tests/test_map_view_args.py and tests/test_gpu_map_view.py."""
import numpy as np

from oracle import oracle as orc

F32 = np.float32


def idx_of_value(value):
    """idx = (int)((float)value * 255): a float multiply, Java's (int) (NaN -> 0, truncation toward zero), clamped to [0, 255]"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(value, dtype=np.float64).astype(F32) * F32(255)
        t = np.where(np.isnan(t), F32(0), t)
        return np.clip(np.trunc(t), 0, 255).astype(np.int32)


def grey_of_idx(idx):
    """g = (int)(255 * (idx / 256f)) in float: white is 254"""
    return (F32(255) * (np.asarray(idx).astype(F32) / F32(256))).astype(np.int32)


def packed_of_grey(g):
    """colorToFloatBits(ratio, ratio, ratio, 1.0f)'s int bits after its & 0xfeffffff mask"""
    g = np.asarray(g).astype(np.uint32)
    return (np.uint32(0xFE000000) | g << np.uint32(16) | g << np.uint32(8) | g).astype(np.uint32)


def log_values(log):
    """value = (double)1.0f - Util.invLogOdds(l), invLogOdds through the oracle's libm once per DISTINCT log-odds value (a map holds
    few: n_free * l_free + n_occ * l_occ) -- neither numpy's exp nor the device's enters the expectation"""
    log = np.asarray(log, dtype=np.float64)
    u, inv = np.unique(log, return_inverse=True)
    L = orc.lib()
    vals = np.array([1.0 - L.orc_inv_log_odds(float(x)) for x in u], dtype=np.float64)
    return vals[inv.reshape(-1)].reshape(log.shape)


def fragile(value):
    """cells whose idx changes when value moves by 4 double ulps either way (a condition on the reference values alone)"""
    value = np.asarray(value, dtype=np.float64)
    lo = hi = value
    for _ in range(4):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    i = idx_of_value(value)
    return (idx_of_value(lo) != i) | (idx_of_value(hi) != i)


def idx_map(data, likelihood):
    """every cell's idx of a downloaded [H][W] array; a log view's inputs must hold no fragile cell"""
    if likelihood:
        return idx_of_value(data)                      # no exp: exact
    v = log_values(data)
    assert not fragile(v).any(), "a fragile cell in the test's inputs: choose another seed"
    return idx_of_value(v)


def expect(idx, rect, d, likelihood, packed):
    """the view of rect = (x0, y0, w, h) at d cells per pixel from the cells' idx [H][W]: ceil(h / d) x ceil(w / d) pixels, ragged last
    row / column; a pixel is the block's minimum idx (log view) or maximum idx (likelihood view)"""
    x0, y0, w, h = rect
    oh, ow = -(-h // d), -(-w // d)
    pad = np.full((oh * d, ow * d), 0 if likelihood else 255, dtype=np.int32)
    pad[:h, :w] = idx[y0:y0 + h, x0:x0 + w]
    blocks = pad.reshape(oh, d, ow, d)
    red = blocks.max(axis=(1, 3)) if likelihood else blocks.min(axis=(1, 3))
    g = grey_of_idx(red)
    return packed_of_grey(g) if packed else g.astype(np.uint8)
