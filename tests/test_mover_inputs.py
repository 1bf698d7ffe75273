"""The evidence that tests/test_gpu_query_movers.py can fail: for every mover x consumer pair it runs, the consumer's expected answer on
the logData before the mover differs from the one on the logData the oracle predicts afterwards, by at least MARGIN cells, records or
poses -- a device that answered from the map as it was would be caught.  Host only: tests/_mover_cases.py and the expectation modules."""
import numpy as np
import pytest

import _mover_cases as mc


def _matrix(shape):
    cons = mc.consumers_of(shape)
    rows = {}
    for name in mc.mover_names(shape):
        before, predicted, _, _ = mc.case_of(shape, name)
        rows[name] = {c: mc.differing(cons[c].expect(before), cons[c].expect(predicted)) for c in mc.CONSUMERS}
    return rows


def _print(shape, rows):
    print(f"\n{shape}: cells, records or poses of each consumer's expected answer that each mover changes")
    for k, c in enumerate(mc.CONSUMERS):
        print(f"  [{k:2d}] {c}")
    print(" " * 46 + "".join(f"{k:6d}" for k in range(len(mc.CONSUMERS))))
    for name, row in rows.items():
        print(f"  {name:44s}" + "".join(f"{row[c]:6d}" for c in mc.CONSUMERS))


@pytest.mark.parametrize("shape", list(mc.SHAPES))
def test_every_pair_the_device_runs_would_catch_a_stale_answer(shape):
    rows = _matrix(shape)
    _print(shape, rows)
    for name, row in rows.items():
        mv = mc.MOVERS[name]
        before, predicted, _, _ = mc.case_of(shape, name)
        if not mv.moves:
            assert np.array_equal(before.view(np.uint64), predicted.view(np.uint64)), (name, "a non-mover leaves logData as it is")
            assert all(v == 0 for v in row.values()), (name, row)
            continue
        for c, changed in row.items():
            if mc.sees(name, c):
                assert changed >= mc.MARGIN, (name, c, changed, "the request does not see the mover: change the request")
        seen = sum(mc.sees(name, c) for c in row)
        assert seen >= 8, (name, seen, "a true mover is seen by at least eight consumers")
    if shape == "64x64":
        for c in mc.CONSUMERS:
            seen = sum(mc.sees(n, c) for n in rows)
            assert seen >= 9, (c, seen, "a consumer is sensitive to at least nine movers")
    assert all(mv in mc.MOVERS and c in mc.CONSUMERS for mv, c in mc.BLIND)
    assert all(mc.sees(mv, c) or mc.consumers_of(shape)[c].field or not mc.MOVERS[mv].moves for mv, c in mc.pairs(shape)), "the device runs no pair that cannot fail"


def test_the_lists_are_the_ones_the_issue_names():
    assert set(mc.CAST_MOVERS) <= set(mc.MOVERS) and len(mc.CAST_MOVERS) == 11
    assert [n for n, mv in mc.MOVERS.items() if not mv.moves] == ["warp_from, compare only", "upload_likelihood"]
    assert mc.mover_names("65x33") == ["upload_log", "update, deferred", "warp_from, add"]
    assert {"warp_from, replace", "warp_from, replace, shifted a cell", "warp_from, add", "warp_from, add, shifted a cell"} <= set(mc.MOVERS)
    cons = mc.consumers_of("64x64")
    assert [c for c in cons if cons[c].field] == ["align"] and sum(mv.field is not None for mv in mc.MOVERS.values()) >= 9
    assert sum(c.table for c in cons.values()) == 3 and sum(c.not_free for c in cons.values()) >= 9 and sum(c.occupied for c in cons.values()) >= 9
    g = mc.grid_of("65x33")
    assert (g.W, g.H) == (65, 33) and g.W % 64 == 1 and g.H % 2 == 1, "one cell in the second 64-bit word of a row, an odd count of rows"
