"""The grid rule of the stage kernels (StageGrid, pbrt-v4_amd/csrc/hip/wf_plan.h; DESIGN.md 4.7 "Stage grids"), asked on the HOST (no GPU)
through Scene.plan("stage_grid:<n_max>:<block>:<per CU>:<CUs>:<rounds>:<cap>") -> wf_scene_plan_query:

    min(ceil(n_max / block), rounds * per_cu * cus)      rounds > 0 and the kernel's occupancy known (per_cu > 0)
    min(ceil(n_max / block), 2048)                       otherwise (the fixed bound of the launches before the rule)

at most `cap` workgroups if one is set, never fewer than one.  The expected values below are worked out by hand from that statement."""
import os

import pytest

from conftest import GOLDEN

BOUND = 2048   # 256 CUs x 8 workgroups: the fixed bound


@pytest.fixture(scope="module")
def grid(wfpt):
    s = wfpt.Scene(path=os.path.join(GOLDEN, "cornell64.pbrt"), spp=1)
    yield lambda n, block=256, per_cu=3, cus=256, rounds=1, cap=0: s.plan("stage_grid:%d:%d:%d:%d:%d:%d" % (n, block, per_cu, cus, rounds, cap))
    s.close()


def test_empty_and_single_item_queues_take_one_workgroup(grid):
    assert grid(0) == 1
    assert grid(1) == 1
    assert grid(0, rounds=0) == 1 and grid(1, rounds=0) == 1


def test_one_block_and_one_more(grid):
    assert grid(256) == 1
    assert grid(257) == 2
    assert grid(1024, block=1024) == 1 and grid(1025, block=1024) == 2   # (the routing pass: 1024 threads)


def test_one_round_and_one_more(grid):
    """a lean shade kernel: 3 workgroups per CU, 256 CUs -> 768 resident"""
    one_round = 768 * 256
    assert grid(one_round - 1) == 768
    assert grid(one_round) == 768
    assert grid(one_round + 1) == 768                  # one persistent round: the 769th block's items go to the grid-stride loop
    assert grid(one_round + 1, rounds=2) == 769        # below two rounds: one workgroup per block
    assert grid(2 * one_round + 1, rounds=2) == 1536
    assert grid(10 ** 9, rounds=4) == 3072
    assert grid(10 ** 9, per_cu=6, rounds=4) == 6144   # whole rounds may exceed the fixed bound


def test_without_rounds_or_occupancy_the_fixed_bound_holds(grid):
    for kw in (dict(rounds=0), dict(per_cu=0), dict(cus=0)):
        assert grid(BOUND * 256, **kw) == BOUND
        assert grid(BOUND * 256 + 1, **kw) == BOUND
        assert grid(BOUND * 256 - 256, **kw) == BOUND - 1
        assert grid(40 * 10 ** 6, **kw) == BOUND


def test_cap(grid):
    assert grid(3 * 256, cap=3) == 3
    assert grid(3 * 256 + 1, cap=3) == 3
    assert grid(2 * 256, cap=3) == 2
    assert grid(100, cap=3) == 1
    assert grid(40 * 10 ** 6, cap=3) == 3
    assert grid(40 * 10 ** 6, rounds=0, cap=3) == 3 and grid(40 * 10 ** 6, per_cu=0, cap=3) == 3
    assert grid(40 * 10 ** 6, cap=10 ** 6) == 768      # a cap above the rule's own bound changes nothing


def test_malformed_keys_are_unknown(wfpt):
    s = wfpt.Scene(path=os.path.join(GOLDEN, "cornell64.pbrt"), spp=1)
    try:
        for key in ("stage_grid:", "stage_grid:1:256:3:256:1", "stage_grid:1:0:3:256:1:0", "stage_grid:-1:256:3:256:1:0", "stage_grid:1:256:3:256:1:0:7"):
            with pytest.raises(wfpt.WfError):
                s.plan(key)
    finally:
        s.close()
