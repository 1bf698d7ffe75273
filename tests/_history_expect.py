"""What the trajectory calls of a gms_slam must return (include/gridmapslam.h "trajectories"), as a host model that never touches them: it
is fed the poses a getter returned after every update and, after every resampling step, whether each filter drew and with which
indices -- and keeps the ring, the lineage rule and the back-trace as the header states them."""
import numpy as np


class HistoryModel:
    def __init__(self, n_filters: int, n_per: int, capacity: int):
        self.S, self.n, self.cap = int(n_filters), int(n_per), int(capacity)
        self.clear()

    def clear(self):
        self.rows = []                                                    # (poses [S][n][3], parents [S][n]) of the kept updates, oldest first
        self.total = 0
        self.lin = np.tile(np.arange(self.n, dtype=np.int32), (self.S, 1))

    @property
    def kept(self) -> int:
        return len(self.rows)

    def update(self, poses):
        """an update returned: the slots' poses as gms_pf_get_poses gave them"""
        self.rows.append((np.array(poses, dtype=np.float32).reshape(self.S, self.n, 3), self.lin.copy()))
        self.rows = self.rows[-self.cap:]
        self.total += 1
        self.lin = np.tile(np.arange(self.n, dtype=np.int32), (self.S, 1))

    def resample(self, did, indices):
        """a resampling step returned: did [S] (gms_pf_did_resample), indices [S][n] filter-local (stale where a filter did not draw)"""
        did = np.asarray(did).reshape(self.S)
        idx = np.asarray(indices).reshape(self.S, self.n)
        for f in range(self.S):
            if did[f]:
                self.lin[f] = self.lin[f][idx[f]]

    def trajectories(self, f: int = 0):
        """(xytheta [kept][n][3], ancestors [kept][n]) of filter f's present particles, oldest first"""
        xy = np.empty((self.kept, self.n, 3), dtype=np.float32)
        anc = np.empty((self.kept, self.n), dtype=np.int32)
        slot = self.lin[f].copy()
        for j in range(self.kept - 1, -1, -1):
            poses, parents = self.rows[j]
            anc[j] = slot
            xy[j] = poses[f][slot]
            slot = parents[f][slot]
        return xy, anc
