"""Replaying a recorded trace through the device path, frame by frame: what GridMapApp.onHandleData does with every
revolution (J/app/GridMapApp.java:133-192) -- de-skew the raw measurements with the frame's odometry (:143-175), then
SLAM.update(z, u) (J/slam/SLAM.java:80-131: motion-model sample per particle, weight, map update at the filter's pose) and
`if (neff < N / 2) resample()` (:185-186).  Here: gms_slam_frame, one call per frame (= gms_map_deskew -> gms_pf_sample_motion ->
gms_slam_update_dev), the scan handed over as the recording's raw host arrays, everything else resident on the device.
ParticleMapsReplay / ParticleMapsBatchReplay are the same for the filter of the reference's own shape, one GridMapData per particle:
gms_slam_frame_per_particle / gms_slam_frame_batch, one call per revolution."""
from __future__ import annotations

import math

import numpy as np

from .gridmap import GridMap, ParticleFilter, SLAMParticleMaps, SLAMParticleMapsBatch
from .synth import dead_reckon
from .trace import Frame


class TraceReplay:
    def __init__(self, grid_map: GridMap, pf: ParticleFilter, start_pose, seed: int = 2024, resample_fraction: float = 0.5,
                 one_call: bool = True):
        self.m, self.pf, self.seed, self.fraction = grid_map, pf, seed, resample_fraction
        self.one_call = one_call        # gms_slam_frame per revolution; False: the three calls it stands for (the same bits)
        self.pose = np.asarray(start_pose, dtype=np.float32)          # dead-reckoned pose of the bootstrap frames
        self.frame_no = 0
        pf.set_poses(np.broadcast_to(self.pose, (pf.n, 3)).copy())    # SLAM.java:65-77: every particle starts at the same pose

    def bootstrap(self, f: Frame):
        """A mapping-only frame: the scan goes into the map at the dead-reckoned pose.  (The reference starts from an empty
        map, whose likelihood field scores every pose alike: 0.1 per beam, GridMap.java:285-286 -- 1e-360 at 360 beams.  A few
        frames of plain mapping give the filter something to localise against.)"""
        self.pose = dead_reckon(self.pose, f.d_center, f.d_theta)
        obs = self.m.deskew(f.angle, f.distance, f.hit, f.d_center, f.d_theta)                     # GridMapApp.java:143-175
        self.m.update(obs, self.pose)                                                              # GridMap.java:173-250
        self.pf.set_poses(np.broadcast_to(self.pose, (self.pf.n, 3)).copy())
        self.frame_no += 1

    def step(self, f: Frame, r01: float):
        """One recorded revolution through the filter (GridMapApp.java:143-192)."""
        integrate = abs(f.d_theta) <= math.radians(30)                                             # SLAM.java:82
        if self.one_call:
            self.pf.slam_frame(f.angle, f.distance, f.hit, f.d_center, f.d_theta, self.seed, self.frame_no, r01, self.fraction, integrate)
        else:
            dev, B = self.m.deskew_dev(f.angle, f.distance, f.hit, f.d_center, f.d_theta)          # :143-175
            self.pf.sample_motion(f.d_center, f.d_theta, self.seed, self.frame_no)                 # SLAM.java:90, 155-163
            self.pf.slam_update_dev(0, dev, B, r01, self.fraction, integrate)                      # :87-131 + GridMapApp.java:185-186
        self.frame_no += 1


class ParticleMapsReplay:
    """The counterpart of TraceReplay for SLAMParticleMaps: every revolution is ONE frame() call (de-skew, update(z, u), the
    resampling rule), nothing read back.  The reference starts every particle at Pose(0, 0, 0) (SLAM.java:65-77); start_pose puts them
    where a recording's drive begins instead."""

    def __init__(self, slam: SLAMParticleMaps, seed: int = 2024, resample_fraction: float = 0.5, start_pose=None, history=None):
        self.slam, self.seed, self.fraction = slam, seed, resample_fraction
        if history is not None:         # keep the particles' paths of the last `history` revolutions (SLAMParticleMaps.set_history)
            slam.set_history(history)
        self.pose = np.zeros(3, dtype=np.float32) if start_pose is None else np.asarray(start_pose, dtype=np.float32)
        self.frame_no = 0
        if start_pose is not None:
            slam.set_poses(np.broadcast_to(self.pose, (slam.num_particles, 3)).copy())

    def bootstrap(self, f: Frame):
        """A mapping-only frame (as TraceReplay.bootstrap): every particle sits at the dead-reckoned pose and integrates the scan into
        its own map there; no motion sample, no resampling.  (Over blank maps a scan of 360 beams weighs every particle 0.1^360 = 0 and
        update() divides 0 by 0, as the reference does: the weights are rewritten by the next update.)"""
        self.pose = dead_reckon(self.pose, f.d_center, f.d_theta)
        self.slam.set_poses(np.broadcast_to(self.pose, (self.slam.num_particles, 3)).copy())
        obs = self.slam.grid_map.deskew(f.angle, f.distance, f.hit, f.d_center, f.d_theta)         # GridMapApp.java:143-175
        self.slam.update(obs, (f.d_center, f.d_theta), sequence=self.frame_no, fetch=False, sample_motion=False)
        self.frame_no += 1

    def step(self, f: Frame, r01: float, fetch: bool = False):
        """One recorded revolution through the filter (GridMapApp.java:143-192)."""
        out = self.slam.frame(f.angle, f.distance, f.hit, f.d_center, f.d_theta, seed=self.seed, sequence=self.frame_no, r01=r01,
                              fraction=self.fraction, fetch=fetch)
        self.frame_no += 1
        return out

    def trajectory(self, which="strongest"):
        """(xytheta [kept][3], shown): where the robot was according to particle `which`, the one whose map view() shows (history=...)"""
        return self.slam.trajectory(which)


class ParticleMapsBatchReplay:
    """S recordings, one per filter of a SLAMParticleMapsBatch, stepped together: every step is ONE frame() call for all of them.
    Frames of unequal measurement counts are padded to the longest and go through `lengths`."""

    def __init__(self, slam: SLAMParticleMapsBatch, seeds=2024, resample_fraction: float = 0.5, start_poses=None, history=None):
        self.slam, self.fraction = slam, resample_fraction
        if history is not None:
            slam.set_history(history)
        S = slam.num_filters
        self.seeds = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint64), (S,)))
        self.frame_no = 0
        if start_poses is not None:
            P = np.asarray(start_poses, dtype=np.float32).reshape(S, 1, 3)
            slam.set_poses(np.ascontiguousarray(np.broadcast_to(P, (S, slam.num_particles, 3))))

    def step(self, frames, r01, fetch: bool = False):
        """frames: S Frame objects, filter f's revolution frames[f]; r01 [S] (or one for all)"""
        S = self.slam.num_filters
        if len(frames) != S:
            raise ValueError(f"step: {len(frames)} frames for {S} filters")
        lengths = np.array([len(f.angle) for f in frames], dtype=np.int32)
        L = int(lengths.max())
        a, d, h = np.zeros((S, L)), np.zeros((S, L)), np.zeros((S, L), dtype=np.uint8)
        for k, f in enumerate(frames):
            a[k, :lengths[k]], d[k, :lengths[k]], h[k, :lengths[k]] = f.angle, f.distance, f.hit
        odo = np.array([(f.d_center, f.d_theta) for f in frames], dtype=np.float64)
        out = self.slam.frame(a, d, h, odo, seeds=self.seeds, sequence=self.frame_no, r01=r01, fraction=self.fraction, lengths=lengths,
                              fetch=fetch)
        self.frame_no += 1
        return out

    def trajectory(self, which="strongest", filter: int = 0):
        """(xytheta [kept][3], shown) of filter `filter`'s particle `which` (history=...)"""
        return self.slam.trajectory(which, filter)
