"""Builds libgridmapslam.so (the HIP C-ABI library) in-tree with hipcc for gfx950."""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libgridmapslam.so")
# gms_fused_kernels.hip is the device translation unit: it includes gms_map_kernels.hip, gms_pf_kernels.hip and gms_slam_kernels.hip;
# gms_query.hip (what the map queries share: checks, bit planes, staging), gms_cast.hip (predicted scans), gms_gain.hip (view gain),
# gms_clearance.hip (clearance fields), gms_reach.hip (cost-to-go fields), gms_frontier.hip (frontier regions), gms_scatter.hip
# (particle seeding), gms_locate.hip (global scan matching), gms_modes.hip (pose modes), gms_beams.hip (the beam sensor model),
# gms_align.hip (continuous scan alignment), gms_rollout.hip (trajectory rollouts), gms_route.hip (routes), gms_warp.hip (maps under a rigid transform)
# gms_skeleton.hip (nearest-obstacle sites and the free-space skeleton) and gms_rooms.hip (rooms and doors) are units of their own, kernels and C-ABI;
# gms_census.hip (the census of a gms_slam's particle maps: counts, consensus, agreement) is a kernel unit whose C-ABI is gms_slam_host.hip's;
# gms_slam_align.hip (the alignment of every particle of a gms_slam on its own field) and gms_slam_beams.hip (the beam sensor model of
# every particle on its own map) are kernel units whose C-ABI is gms_slam_host.hip's;
# gms_probe.h is the device header the casts and the beam models share, gms_beams_device.h the ONE workgroup body of the two beam models
# (each unit supplies its source of occupancy bits), gms_align_device.h the two alignment units' (staging, evaluation, step, store),
# gms_nearest_device.h the ONE separable nearest-obstacle transform of gms_clearance.hip and gms_skeleton.hip (each unit instantiates its policy),
# gms_relax_device.h the ONE tile relaxation of gms_reach.hip and gms_rooms.hip (round body, sweep, marks, the host's round loop; each unit
# instantiates its policy), gms_regions.h the union, the ONE tile labelling of gms_frontier.hip and gms_rooms.hip, the group loop and the reductions,
# gms_slam_device.h what the device unit, gms_slam_align.hip and gms_slam_beams.hip share of a gms_slam's kernels (the per-particle prologue)
SOURCES = ["gms_host.hip", "gms_slam_host.hip", "gms_fused_kernels.hip", "gms_query.hip", "gms_cast.hip", "gms_gain.hip", "gms_clearance.hip",
           "gms_reach.hip", "gms_frontier.hip", "gms_scatter.hip", "gms_locate.hip", "gms_modes.hip", "gms_beams.hip", "gms_align.hip",
           "gms_slam_align.hip", "gms_slam_beams.hip", "gms_rollout.hip", "gms_route.hip", "gms_warp.hip", "gms_census.hip", "gms_skeleton.hip",
           "gms_rooms.hip"]
# -ffp-contract=off: the reference (JVM) never fuses a multiply with an add; parity depends on it.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
         "-shared", "-fvisibility=hidden", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]
# Kernel-argument preload, for the device translation unit only: gfx950 delivers the head of the kernel-argument segment in user
# SGPRs with the wave's launch (14 dwords beside the segment's pointer), so a kernel's first loads and branches do not wait for a
# scalar load of their addresses.  A structure passed by value ends the preloaded run, which is why the step kernels take their
# descriptors last (k_score_c's argument-order note).  The other units keep the compiler's default.
UNIT_FLAGS = {"gms_fused_kernels.hip": ["-mllvm", "-amdgpu-kernarg-preload-count=16"]}


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def extra_flags() -> list:
    return os.environ.get("GMS_EXTRA_FLAGS", "").split()      # experiments only (e.g. -DRC_RAYS=4, -DGMS_STAMPS)


def source_hash() -> str:
    """sha256 (16 hex digits) over the library's sources -- csrc/* and the public header, in name order -- and, when
    GMS_EXTRA_FLAGS is set, over those flags as well: an instrumented or experimental build carries another hash than the
    product build of the same sources, so neither is ever taken for the other (gms_build_info(), the up-to-date check)."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))) + [os.path.join(ROOT, "include", "gridmapslam.h")]
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    for unit in sorted(UNIT_FLAGS):
        h.update(b"\0unit\0" + unit.encode() + b"\0" + " ".join(UNIT_FLAGS[unit]).encode())
    extra = extra_flags()
    if extra:
        h.update(b"\0flags\0" + " ".join(extra).encode())
    return h.hexdigest()[:16]


def built_hash(lib: str = LIB) -> str | None:
    """the source hash a built library carries (the string gms_build_info() returns), read from the file itself"""
    try:
        blob = open(lib, "rb").read()
    except OSError:
        return None
    i = blob.find(b"GMS_SOURCE_HASH=")
    return blob[i + 16:i + 32].decode("ascii", "replace") if i >= 0 else None


def needs_build() -> bool:
    return built_hash() != source_hash()


def build(force: bool = False, verbose: bool = False) -> str:
    """Compiles the library unless the in-tree one was built from exactly these sources; says which on stderr, with the hash
    (the same string gms_build_info() returns at run time, so a log shows which binary ran)."""
    want = source_hash()
    if not force and built_hash() == want:
        print(f"libgridmapslam: reused {want} (in-tree build of these sources)", file=sys.stderr)
        return LIB
    os.makedirs(LIBDIR, exist_ok=True)
    extra = extra_flags()
    # A unit with flags of its own cannot share a command line with the others, so the library is built in three steps: such units to
    # objects one by one, the other units to objects in one command, then the link (hipcc takes a command line of objects alone as
    # one: beside a source file it reads every input as HIP source).  The objects live in a temporary directory of this build alone
    # and go with it; the library is linked there too and moved into place whole, so two builds at once never share a file.
    common = [hipcc()] + [a for a in FLAGS if a != "-shared"] + extra
    common += [f'-DGMS_SOURCE_HASH="{want}"', "-I", os.path.join(ROOT, "include"), "-I", CSRC]
    cmds = [common + UNIT_FLAGS[s] + ["-c", os.path.join(CSRC, s)] for s in SOURCES if s in UNIT_FLAGS]
    cmds.append(common + ["-c"] + [os.path.join(CSRC, s) for s in SOURCES if s not in UNIT_FLAGS])
    objects = [os.path.splitext(s)[0] + ".o" for s in SOURCES]
    # (the extra flags reach the link as well: one that matters there, such as -g or -fsanitize, is not dropped)
    cmds.append([hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared", "-fvisibility=hidden", "-Wno-unused-command-line-argument"]
                + extra + objects + ["-o", os.path.basename(LIB)])
    with tempfile.TemporaryDirectory(prefix=".build-", dir=LIBDIR) as tmp:
        for cmd in cmds:
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            subprocess.check_call(cmd, cwd=tmp)
        os.replace(os.path.join(tmp, os.path.basename(LIB)), LIB)
    print(f"libgridmapslam: built {want}" + (f" (extra flags: {' '.join(extra)})" if extra else ""), file=sys.stderr)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
