"""CPU: the arithmetic of tools/flush_sim.py (the flush-policy screen) on logs made by hand."""
import importlib.util
import os

from _util import REPO

_spec = importlib.util.spec_from_file_location("flush_sim", os.path.join(REPO, "tools", "flush_sim.py"))
FS = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(FS)


def _tag(i, j):
    return i << 8 | j


def test_parse_log_and_lane_steps():
    # one pixel-sample: connectable eye vertices 2, 3; light vertices 2; s = 0 source 3; nL = 3
    log = [-1, 0b1100, 0b100, -2, 0b1000, 3,
           _tag(1, 1), 4, 1, _tag(2, 1), 7, 2, _tag(3, 2), 5, 0,
           -1, 0, 0, -2, 0, 1]
    recs = FS.parse_log(log)
    assert len(recs) == 2
    assert recs[0]["rays"] == {(1, 1): (4, 1), (2, 1): (7, 2), (3, 2): (5, 0)} and recs[1]["rays"] == {}
    s0, j1, i1, pairs = FS.lane_steps(recs[0])
    assert s0 == [(3, 0)]
    assert j1 == [(1, 1), (2, 1), (3, 1)]      # the camera vertex first, then the connectable ones
    assert i1 == [(1, 2)]
    assert pairs == [(2, 2), (3, 2)]
    assert FS.lane_steps(recs[1]) == [[], [], [], []]   # nL = 1: no fresh light sample
    assert FS.lane_steps(None) == [[], [], [], []]


def test_item_pushes_order_and_next_bound():
    a = {"cE": 0b1100, "cL": 0b100, "sE": 0b1000, "nL": 3, "rays": {(1, 1): (4, 1), (2, 1): (7, 2), (3, 2): (5, 0)}}
    b = {"cE": 0b100, "cL": 0, "sE": 0, "nL": 2, "rays": {(1, 1): (1, 0), (2, 1): (2, 0)}}
    steps = FS.item_pushes([[a, b] + [None] * 62])
    # s = 0: one step (lane a alone), no ray; j = 1: three steps, lane b has two; i = 1: one; pairs: two
    assert [len(p) for p, _ in steps] == [0, 2, 2, 0, 0, 0, 1]
    assert steps[1][0] == [(4, 1), (1, 0)] and steps[2][0] == [(7, 2), (2, 0)]   # lane order within a step
    assert steps[6][0] == [(5, 0)]
    assert [nxt for _, nxt in steps] == [64, 2, 1, 64, 64, 1, 64]


def test_drain():
    assert FS.drain([3, 9, 1]) == 9 and FS.drain([]) == 0
    # 64 rays of 2 steps and one of 10, idle threshold 16: with nothing queued the wave waits for the longest
    assert FS.drain([2] * 63 + [10], 16) == 10
    # 66 rays: two wait; after 2 steps 63 lanes are idle (>= 16): one refill round, then 5 more steps
    assert FS.drain([2] * 63 + [10] + [5, 5], 16) == 2 + 1 + max(10 - 2, 5)
    # below the threshold no refill happens until enough lanes have ended
    assert FS.drain([1] * 10 + [4] * 54 + [3], 16) == 4 + 1 + 3
    assert FS.drain([1] * 16 + [4] * 48 + [3], 16) == 1 + 1 + 3
    # fewer than 64 rays never refill
    assert FS.drain([5, 1], 8) == 5


def test_replay_policies():
    one = (3, 1)
    # 5 steps of 40 pushes each, every lane's list still full after each but the last
    steps = [([one] * 40, 64)] * 4 + [([one] * 40, 64)]
    cur = FS.replay(steps, "current")
    # 40, 80 -> flush 64 (16 left), 56, 96 -> flush 64 (32), 72 -> flush 64 (8), the end flushes 8
    assert (cur["flushes"], cur["rays"], cur["node"], cur["both"]) == (4, 200, 4 * 3, 4 * 4)
    ref = FS.replay(steps, "refill", idle=16)
    # 80 -> drain 80, 80 -> drain 80, the end drains 40: 3 + 1 + 3 steps each for the first two
    assert (ref["flushes"], ref["rays"], ref["node"]) == (3, 200, 7 + 7 + 3)
    late = FS.replay(steps, "late", idle=16)
    # 40 + 64 <= 128; 80 + 64 > 128 -> drain 80; 40; 80 -> drain 80; the end drains 40
    assert (late["flushes"], late["rays"]) == (3, 200)
    # a small bound for the next step lets the ring fill further
    steps = [([one] * 60, 4), ([one] * 4, 4), ([one] * 4, 64)]
    late = FS.replay(steps, "late", idle=16)
    assert (late["flushes"], late["rays"]) == (1, 68)   # 60 + 4, 64 + 4 <= 128; 68 + 64 > 128 -> drain 68
    assert FS.summarise([steps, steps], "late")[:2] == (1.0, 68.0)
