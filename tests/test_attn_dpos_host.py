"""Host-side checks of the linear_pos gradient path (csrc/attn_dpos.hip): a3t_attn_bwd_dpos_plan / _ws, the one place its tiling
is decided, through the library as built (no GPU: the plan is pure host code and assumes 256 compute units without a device)."""
import pytest

CUS = 256
MAX_ROWS = 192      # the kernel's tallest tile: three 64-column panels of the [k][m] operand per LDS stage (DP_NPA)
# configs[1], configs[3], the cases of tests/test_gpu_attn_dpos.py (five with groups of one, then the two whose groups hold two elements)
SHAPES = [(32, 2, 1120, 192), (16, 4, 1800, 128),
          (3, 2, 40, 32), (5, 1, 72, 192), (2, 2, 136, 128), (3, 2, 328, 64), (4, 2, 168, 96),
          (141, 2, 40, 32), (129, 2, 136, 128)]


@pytest.fixture(scope="module")
def ops():
    from a3t_amd import build, ops
    build.build(verbose=False)
    return ops


@pytest.mark.parametrize("B,H,T,dk", SHAPES)
def test_plan_covers_the_problem_in_one_round(ops, B, H, T, dk):
    plan = ops.attn_bwd_dpos_plan(B, H, T, dk)
    assert plan is not None
    rows, tiles, group, grid = plan
    assert rows % 32 == 0 and 32 <= rows <= MAX_ROWS
    assert tiles * rows >= T and (tiles - 1) * rows < T, "every tile holds rows"
    assert group >= 1
    groups = -(-B // group)
    assert (groups - 1) * group < B <= groups * group, "the groups cover B; the last one is short when B is no multiple"
    if B % group:
        assert B - (groups - 1) * group < group
    assert grid == tiles * H * groups and grid <= CUS
    assert ops.attn_bwd_dpos_ws(B, H, T, dk) >= groups * T * H * dk


def test_plan_keeps_groups_of_two_in_the_test_table(ops):
    """The hand-over between batch elements inside a workgroup needs a group of more than one element: two cases of the GPU table
    have one, and one of them a short last group."""
    assert ops.attn_bwd_dpos_plan(141, 2, 40, 32)[2] == 2 and 141 % 2 == 1
    assert ops.attn_bwd_dpos_plan(129, 2, 136, 128)[2] == 2


@pytest.mark.parametrize("B,H,T,dk", [(2, 2, 44, 32), (2, 2, 1124, 192), (2, 2, 40, 160), (2, 2, 40, 224), (2, 2, 0, 32), (2, 2, 40, 48),
                                      (0, 2, 40, 32), (2, 2, 40, 0)])
def test_plan_refuses(ops, B, H, T, dk):
    assert ops.attn_bwd_dpos_plan(B, H, T, dk) is None
    assert ops.attn_bwd_dpos_ws(B, H, T, dk) == 0


def test_plan_refuses_operands_beyond_32_bit_offsets(ops):
    assert ops.attn_bwd_dpos_plan(1, 1, 32768, 32) is None          # T (T + 1) 2 bytes >= 2 GiB
    assert ops.attn_bwd_dpos_plan(1, 1, 16384, 32) is not None


def test_exports_and_wrappers(ops):
    from a3t_amd import _lib
    for name, nargs in (("a3t_attn_bwd_dpos", 13), ("a3t_attn_bwd_dpos_ws", 4), ("a3t_attn_bwd_dpos_plan", 5)):
        assert name in _lib.EXPORTS and len(_lib._SIGS[name]) == nargs
    assert callable(ops.attn_bwd_dpos)
