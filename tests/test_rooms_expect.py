"""The plain restatement of "rooms and doors" (tests/_rooms_expect.py) against answers written out by hand.  No device."""
import numpy as np

import _rooms_expect as rx

NONE, FAR = 0xFFFFFFFF, 0xFFFF


def test_blocked_is_the_disc_around_every_obstacle():
    log = np.full((9, 9), rx.L_FREE)
    log[4, 4] = rx.L_OCC
    b = rx.blocked(log, 2, False)
    # d2 <= 4: the cell, its axis neighbours at 1 and 2, its diagonal neighbours (d2 = 2); (1, 2) has d2 = 5
    assert sorted(map(tuple, np.argwhere(b).tolist())) == sorted([(4, 4), (3, 4), (5, 4), (4, 3), (4, 5), (2, 4), (6, 4), (4, 2), (4, 6), (3, 3), (3, 5),
                                                                 (5, 3), (5, 5)])
    assert rx.blocked(log, 0, False).sum() == 1 and not rx.blocked(np.full((3, 3), rx.L_FREE), 5, True).any()
    log[0, 0] = np.nan                                                          # NaN, 0 and -0.0: obstacles under NOT_FREE alone
    log[0, 8] = 0.0
    log[8, 0] = -0.0
    assert rx.blocked(log, 0, True).sum() == 4 and rx.blocked(log, 0, False).sum() == 1


def test_two_boxes_and_a_three_cell_gap_by_hand():
    """W = 46, H = 24, occupied but for box A = x 2 .. 21, box B = x 23 .. 42 (both y 2 .. 21) and the gap (22, 10 .. 12).  core = 2
    blocks d2 <= 4.  Away from the gap a box's core is the cells 3 or more from every wall: x 4 .. 19, y 4 .. 19 = 256 cells.  Beside
    the gap: (20, y) is 2 from the wall column, so it is a core cell iff (22, y) is free: y = 10, 11, 12; (21, y) is 1 from it, blocked iff
    one of (22, y - 1 .. y + 1) is a wall: only (21, 11) is a core cell; (22, 11) has (22, 9) at d2 = 4: blocked.  So two cores of 260 cells,
    anchors (4, 4) = 188 and (25, 4) = 209.  inflate = 0: every free cell is traversable.  The gap cells: (22, 11) is one axis step from
    (21, 11) and from (23, 11): 5 against 5, the smaller anchor takes it; (22, 10) and (22, 12) are one diagonal step from either (both
    squeezed cells are free): 7 against 7, again A.  A has 400 + 3 cells, B 400.  Contacts (22, y) | (23, y), y = 10 .. 12: count 3, box
    x 22 .. 23, y 10 .. 12, sum_x2 = 3 * 45 = 135, sum_y2 = 2 * 33 = 66.  The deepest cells are the boxes' corners, two diagonal steps
    from the core: 14."""
    e = rx.expect(rx.two_boxes(), core=2, inflate=0, not_free=False)
    assert e["n_rooms"] == 2 and e["n_doors"] == 1
    a, b = e["rooms"]
    assert (a["anchor_x"], a["anchor_y"], a["core_count"], a["count"], a["doors"], a["max_depth"]) == (4, 4, 260, 403, 1, 14)
    assert (b["anchor_x"], b["anchor_y"], b["core_count"], b["count"], b["doors"], b["max_depth"]) == (25, 4, 260, 400, 1, 14)
    assert (a["min_x"], a["min_y"], a["max_x"], a["max_y"]) == (2, 2, 22, 21) and (b["min_x"], b["min_y"], b["max_x"], b["max_y"]) == (23, 2, 42, 21)
    assert (a["sum_x"], a["sum_y"]) == (20 * 230 + 3 * 22, 20 * 230 + 33) and (b["sum_x"], b["sum_y"]) == (20 * 650, 20 * 230)
    d = e["doors"][0]
    assert (d["a"], d["b"], d["count"]) == (188, 209, 3)
    assert (d["min_x"], d["min_y"], d["max_x"], d["max_y"], d["sum_x2"], d["sum_y2"]) == (22, 10, 23, 12, 135, 66)
    lab, dep = e["labels"], e["depth"]
    assert (lab[2:22, 2:23][lab[2:22, 2:23] != NONE] == 188).all() and (lab[10:13, 22] == 188).all() and (lab[2:22, 23:43] == 209).all()
    assert (lab == NONE).sum() == 46 * 24 - 803 and (dep[lab == NONE] == FAR).all()
    assert dep[11, 22] == 5 and dep[10, 22] == 7 and dep[12, 22] == 7 and dep[2, 2] == 14 and dep[11, 21] == 0 and dep[10, 21] == 5
    # the rectangle is cut out of the same field
    r = rx.expect(rx.two_boxes(), core=2, inflate=0, not_free=False, rect=(20, 9, 5, 3))
    assert np.array_equal(r["labels"], lab[9:12, 20:25]) and np.array_equal(r["depth"], dep[9:12, 20:25])


def test_the_middle_of_a_symmetric_corridor_goes_to_the_smaller_anchor():
    """Rooms x 1 .. 9 and x 21 .. 29 (y 3 .. 11), the corridor (10 .. 20, 7).  core = 2: the cores are x 3 .. 7 / 23 .. 27, y 5 .. 9 and
    the cell in front of the opening, (8, 7) / (22, 7): 26 cells, anchors (3, 5) = 158 and (23, 5) = 178.  (15, 7) is seven axis steps
    from (8, 7) and from (22, 7): 35 against 35, so it goes left.  Left: 81 + 6 cells, right: 81 + 5.  The one contact is
    (15, 7) | (16, 7)."""
    e = rx.expect(rx.corridor(), core=2, inflate=0, not_free=False)
    assert e["rooms"]["core_count"].tolist() == [26, 26] and e["rooms"]["count"].tolist() == [87, 86]
    assert e["labels"][7, 15] == 158 and e["labels"][7, 16] == 178 and e["depth"][7, 15] == 35 and e["depth"][7, 16] == 30
    d = e["doors"]
    assert len(d) == 1 and (d["a"][0], d["b"][0], d["count"][0], d["min_x"][0], d["max_x"][0], d["min_y"][0], d["max_y"][0]) == (158, 178, 1, 15, 16, 7, 7)
    assert (d["sum_x2"][0], d["sum_y2"][0]) == (31, 14)
    # the right room two rows taller: its core starts at y = 3, anchor (23, 3) = 116 < 158, and now the middle goes right
    e = rx.expect(rx.corridor(tall_right=True), core=2, inflate=0, not_free=False)
    assert e["labels"][7, 15] == 116 and e["labels"][7, 14] == 158 and e["rooms"]["count"].tolist() == [99 + 6, 81 + 5]
    assert (e["doors"]["a"][0], e["doors"]["b"][0], e["doors"]["sum_x2"][0]) == (116, 158, 29)


def test_min_core_max_cost_and_corner_cutting():
    # min_core above one core's size: that core is grown into by the other; above both: no room at all
    log = rx.two_boxes()
    rx.carve(log, 23, 2, 42, 21, rx.L_OCC)
    rx.carve(log, 23, 7, 30, 15)                                                # the right box shrunk to 8 x 9: core 4 x 5 = 20 cells and the gap's 4
    small = rx.expect(log, core=2, inflate=0, not_free=False)
    assert small["n_rooms"] == 2 and small["rooms"]["core_count"].tolist() == [260, 24]
    one = rx.expect(log, core=2, inflate=0, not_free=False, min_core=25)
    assert one["n_rooms"] == 1 and one["n_doors"] == 0 and one["rooms"]["count"][0] == 403 + 72 and (one["labels"][7:16, 23:31] == 188).all()
    assert rx.expect(log, core=2, inflate=0, not_free=False, min_core=1000)["n_rooms"] == 0
    # max_cost: the corridor cut part-way; beyond the cut NONE, and the door is gone
    e = rx.expect(rx.corridor(), core=2, inflate=0, not_free=False, max_cost=20)
    assert e["n_doors"] == 0 and (e["labels"][7, 13:18] == NONE).all() and e["labels"][7, 12] == 158 and e["labels"][7, 18] == 178
    # two free areas touching only diagonally between two blocked cells: not grown across
    log = rx.walls(20, 12)
    rx.carve(log, 1, 1, 9, 5)
    rx.carve(log, 10, 6, 16, 10)                                                # (9, 5) and (10, 6) touch diagonally; (10, 5) and (9, 6) are walls
    e = rx.expect(log, core=1, inflate=0, not_free=False, min_core=8)
    assert e["n_rooms"] == 2 and e["n_doors"] == 0, "two rooms touching only diagonally have no door"
    assert e["rooms"]["core_count"].tolist() == [7 * 3, 5 * 3] and e["rooms"]["count"].tolist() == [9 * 5, 7 * 5]
    e = rx.expect(log, core=1, inflate=0, not_free=False, min_core=20)          # the right core does not qualify, and nothing grows across the corner
    assert e["n_rooms"] == 1 and (e["labels"][6:11, 10:17] == NONE).all() and (e["labels"][1:6, 1:10] == 2 * 20 + 2).all()
