"""Routes (include/gridmapslam.h "routes") restated in plain Python and numpy: the descent written out anew (gridmap.descend() is the
tests' second yardstick, not called here), VISIBLE as a brute-force loop over the bounding box with the inequality in Python
integers, the pulling loop literal.  visible_box() is the same brute force with the bounding box as one int64 numpy array -- every
value below 2^63, so exact -- for the device tests' many look-ups; tests/test_route_definition.py holds the two against each other."""
import numpy as np

from gridmap_slam_robot_amd._lib import ROUTE_DTYPE

FAR = 0xFFFF
CLEAR_FAR = 0xFFFF
AXIS, DIAG = 5, 7
NO_PATH, BROKEN, CELLS_CUT, WAYPOINTS_CUT, MISMATCH = 1, 2, 4, 8, 16
ORDER = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))        # E, N, W, S, NE, NW, SW, SE; north is y + 1


def descent(field, start, max_cells):
    """(cells, flags, start_cost, end_cost) of one start over field [H][W]"""
    f = np.asarray(field)
    H, W = f.shape
    x, y = int(start[0]), int(start[1])
    on = lambda px, py: 0 <= px < W and 0 <= py < H
    if not on(x, y):
        return [], NO_PATH, FAR, FAR
    if int(f[y, x]) == FAR:
        return [], NO_PATH, FAR, FAR
    cells, flags, start_cost = [(x, y)], 0, int(f[y, x])
    while int(f[y, x]) != 0:
        cur, nxt = int(f[y, x]), None
        for dx, dy in ORDER:
            nx, ny = x + dx, y + dy
            if not on(nx, ny) or int(f[ny, nx]) == FAR:
                continue
            if int(f[ny, nx]) + (DIAG if dx and dy else AXIS) != cur:
                continue
            if dx and dy and (not on(nx, y) or not on(x, ny) or int(f[y, nx]) == FAR or int(f[ny, x]) == FAR):
                continue
            nxt = (nx, ny)
            break
        if nxt is None:
            flags |= BROKEN
            break
        if len(cells) == max_cells:
            flags |= CELLS_CUT
            break
        x, y = nxt
        cells.append(nxt)
    return cells, flags, start_cost, int(f[y, x])


def visible(blocked, a, b):
    """VISIBLE(a, b), literally: every cell of the bounding box inside the closed band is not blocked"""
    (ax, ay), (bx, by) = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    dx, dy = bx - ax, by - ay
    for y in range(min(ay, by), max(ay, by) + 1):
        for x in range(min(ax, bx), max(ax, bx) + 1):
            if 2 * abs((x - ax) * dy - (y - ay) * dx) <= abs(dx) + abs(dy) and blocked[y][x]:
                return False
    return True


def visible_box(blocked, a, b):
    """the same predicate with the bounding box as one array"""
    (ax, ay), (bx, by) = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    dx, dy = bx - ax, by - ay
    x0, x1, y0, y1 = min(ax, bx), max(ax, bx), min(ay, by), max(ay, by)
    xs = np.arange(x0, x1 + 1, dtype=np.int64)[None, :]
    ys = np.arange(y0, y1 + 1, dtype=np.int64)[:, None]
    band = 2 * np.abs((xs - ax) * dy - (ys - ay) * dx) <= abs(dx) + abs(dy)
    return not bool((band & np.asarray(blocked)[y0:y1 + 1, x0:x1 + 1]).any())


def pull(path, blocked, look, max_waypoints, see=visible_box):
    """(waypoints, flags) of one descended path"""
    if not path:
        return [], 0
    w, flags, i = [path[0]], 0, 0
    while i < len(path) - 1:
        if len(w) == max_waypoints:
            flags |= WAYPOINTS_CUT
            break
        j = min(i + look, len(path) - 1)
        while j > i and not see(blocked, path[i], path[j]):
            j -= 1
        if j == i:
            j = i + 1
            flags |= MISMATCH
        w.append(path[j])
        i = j
    return w, flags


def expect(field, blocked, starts, look, max_cells, max_waypoints, clear=None, see=visible_box):
    """(records [P], the waypoint lists, the cell lists) of the starts [P][2]"""
    starts = np.asarray(starts, dtype=np.int64).reshape(-1, 2)
    rec = np.zeros(len(starts), dtype=ROUTE_DTYPE)
    ways, paths = [], []
    for p, s in enumerate(starts):
        cells, flags, start_cost, end_cost = descent(field, s, max_cells)
        w, more = pull(cells, blocked, look, max_waypoints, see)
        min_d2, at = CLEAR_FAR, 0
        if clear is not None and cells:
            d2 = [int(clear[y][x]) for x, y in cells]
            min_d2 = min(d2)
            at = d2.index(min_d2)
        end = cells[-1] if cells else (int(s[0]), int(s[1]))
        rec[p] = (len(cells), len(w), start_cost, end_cost, min_d2, flags | more, at, end[0], end[1], 0)
        ways.append(w)
        paths.append(cells)
    return rec, ways, paths


def same_lists(got, n, want, where=""):
    """got [P][cap][2] holds want's lists in front of the counts n"""
    for p, w in enumerate(want):
        assert int(n[p]) == len(w), f"{where}: start {p}: {int(n[p])} entries, {len(w)} expected"
        assert np.array_equal(np.asarray(got[p][:len(w)]).reshape(-1, 2), np.asarray(w, dtype=np.int64).reshape(-1, 2)), f"{where}: start {p}"
