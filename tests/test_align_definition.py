"""The definition of the continuous scan alignment itself (include/gridmapslam.h "continuous scan alignment"), checked on the restatement
(tests/_align_expect.py) without a device, so that the device's equality with the restatement means something: J is the derivative of
the interpolated field M, the iteration pulls poses in on a map that is not square, that map's geometry is one the tests can tell from
its transpose, and H is a Gram matrix.  Run with -s for the measured figures (DESIGN.md section 4n quotes them)."""
import numpy as np

import _align_expect as ax
from oracle import oracle as orc

RES, SCAN = ax.RES, ax.SCAN
W, H = ax.NS_W, ax.NS_H
F = float(np.float32(RES)), float(np.float32(ax.NS_POS[0])), float(np.float32(ax.NS_POS[1]))      # the handle's floats, widened


def test_j_is_the_derivative_of_the_interpolated_field():
    """For one beam S = M and g_k = J_k (1 - M), so J_k = g_k / (1 - S): each hit beam's J at one perturbed pose against a central
    difference of S with h = 2^-9 in each float pose component (x and y times res: per cell).  Only beams whose end point stays in
    one cell over all six stepped poses count.  M is linear in x and in y inside a cell: 1e-9; in theta the difference's second-order
    term and the float-rounded trig remain: 1e-2, where a wrong sign or exchanged ax / ay would give an error of order 1.
    Measured at this pose: 87 of 115 beams kept, 1.7e-12, 1.0e-12 and 1.6e-3.  The theta figure is the difference's own noise over
    max(1e-3, |J|) and so depends on the pose: where a kept beam's |J2| lies under the floor (3.3e-4 for beam 105 at
    perturbed(true, 1)[0]) an absolute error of 1.8e-5 reads as 1.8e-2."""
    g, _, lik, tr = ax.room_ns()
    scan = tr.scans[SCAN]
    pose = ax.perturbed(tr.poses[SCAN], 37)[0]
    h = 2.0 ** -9
    stepped = []
    for k in range(3):
        for sgn in (1.0, -1.0):
            p = [float(v) for v in pose]
            p[k] = float(np.float32(p[k] + sgn * h))                            # a pose of floats: the quotient below takes the step made
            stepped.append(p)

    def cell(p, b):
        c, s = orc.pose_trig(np.float32(p[2]))
        gu, gv = ax.grid_uv(float(scan["local_x"][b]), float(scan["local_y"][b]), c, s, p[0], p[1], *F)
        return ax._floor(gu), ax._floor(gv)

    hits = np.flatnonzero(scan["hit"])
    err, kept = [], 0
    for b in hits:
        one = scan[b:b + 1]
        Hm, gk, S, n = ax.evaluate(lik, W, H, *F, one, pose)
        if n != 1 or S == 1.0 or any(cell(p, b) != cell(pose, b) for p in stepped):
            continue
        ev = [ax.evaluate(lik, W, H, *F, one, p) for p in stepped]
        if any(e[3] != 1 for e in ev):
            continue
        kept += 1
        J = [v / (1.0 - S) for v in gk]
        fd = [(ev[2 * k][2] - ev[2 * k + 1][2]) / (stepped[2 * k][k] - stepped[2 * k + 1][k]) * (F[0] if k < 2 else 1.0) for k in range(3)]
        err.append([abs(fd[k] - J[k]) / max(1e-3, abs(J[k])) for k in range(3)])
    worst = np.max(np.array(err), axis=0)
    print(f"J against a central difference of S: {kept} of {len(hits)} hit beams kept, worst relative error x {worst[0]:.2e}, "
          f"y {worst[1]:.2e}, theta {worst[2]:.2e}")
    assert kept >= 60
    assert worst[0] <= 1e-9 and worst[1] <= 1e-9 and worst[2] <= 1e-2


def test_restatement_pulls_perturbed_poses_towards_the_true_one_on_the_map_that_is_not_square():
    """8 iterations with the default parameters, 24 starts: both medians fall (DESIGN.md section 4n has the figures)"""
    g, _, lik, tr = ax.room_ns()
    true = tr.poses[SCAN].astype(np.float64)
    start = ax.perturbed(true, 24)
    out, rec = ax.align(lik, W, H, RES, *ax.NS_POS, tr.scans[SCAN], start, ax.default_params())
    t0, t1 = np.hypot(*(start[:, :2] - true[:2]).T), np.hypot(*(out[:, :2] - true[:2]).T)
    r0, r1 = np.abs(start[:, 2] - true[2]), np.abs(out[:, 2] - true[2])
    print(f"median translation error {np.median(t0) / RES:.3f} -> {np.median(t1) / RES:.3f} cells, "
          f"median heading error {np.degrees(np.median(r0)):.3f} -> {np.degrees(np.median(r1)):.3f} degrees, "
          f"status 0 / 1: {int((rec['status'] == 0).sum())} / {int((rec['status'] == 1).sum())}")
    assert np.median(t1) < np.median(t0) and np.median(r1) < np.median(r0)
    assert np.median(rec["score"]) > np.median(rec["score0"]) and (rec["n_used"] > 0).all() and np.isin(rec["status"], (0, 1)).all()


def test_the_geometry_tells_w_from_h_and_pos_x_from_pos_y():
    """what tests/test_gpu_align_shapes.py relies on, checked where no device is: on both maps that are not square the restatement
    with W and H exchanged, or with the origin's components exchanged, ends at other poses (on the square room of
    tests/test_gpu_align.py both exchanges are the identity)"""
    for Wm, Hm, pos in ((W, H, ax.NS_POS), (H, W, ax.NS_POS[::-1])):
        for iters in (1, 8):
            _, _, n_wh, n_pos = ax.discriminating_case(Wm, Hm, pos, iters)
            print(f"{Wm} x {Hm} at {pos}, iters {iters}: {n_wh} of 37 poses differ with W and H exchanged, {n_pos} with pos_x and pos_y exchanged")


def test_h_is_a_gram_matrix():
    """H = sum J J^T over the used beams: non-negative diagonal and leading 2 x 2 minor, the 3 x 3 matrix symmetric positive
    semi-definite up to rounding (smallest eigenvalue >= -1e-9 times the largest)"""
    g, _, lik, tr = ax.room_ns()
    for pose in ax.perturbed(tr.poses[SCAN], 4, seed=23):
        Hm, _, S, n = ax.evaluate(lik, W, H, *F, tr.scans[SCAN], pose)
        assert n > 100
        assert Hm[0] >= 0.0 and Hm[3] >= 0.0 and Hm[5] >= 0.0 and Hm[0] * Hm[3] - Hm[1] * Hm[1] >= 0.0
        ev = np.linalg.eigvalsh(np.array([[Hm[0], Hm[1], Hm[2]], [Hm[1], Hm[3], Hm[4]], [Hm[2], Hm[4], Hm[5]]]))
        assert ev[-1] > 0.0 and ev[0] >= -1e-9 * ev[-1], ev
