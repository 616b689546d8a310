"""CPU: the stage checks of tests/mlp_block_reference.py accept a faithful fp32 / bf16 emulation of the block-form MLP kernels
(csrc/vsde_mlp.hip, BLK == 1 and BLK == 2) at every (shape, class) case of tests/test_mlp_block_ops_gpu.py, hold their
ambiguous-share conditions there, and reject each of twelve injected defects -- every defect test names the check that catches it."""
import pytest
import torch

import mlp_block_reference as br

ALL = [pytest.param(blk, case, id=br.case_id(blk, case)) for blk in (1, 2) for case in br.CASES]
_CACHE: dict = {}


def _case(blk, case):
    """Operands and the outcome of the correct emulation, built once per case and left unchanged."""
    key = (blk, case)
    if key not in _CACHE:
        ops = br.build_case(blk, case, seed=1000 * blk + br.CASES.index(case))
        _CACHE[key] = (ops, br.check_case(ops, br.emulate, key=br.case_id(blk, case)))
    return _CACHE[key]


@pytest.mark.parametrize("blk,case", ALL)
def test_checks_accept_the_emulation_and_hold_their_share_conditions(blk, case):
    ops, res = _case(blk, case)
    br.assert_case(res, br.case_id(blk, case))
    # the checks every case must have made
    want = {"x1" if blk == 1 else "x1(W_o)", "select", "scm1"} | ({"probe"} if blk == 2 else set())
    if not case[6]:
        want |= {"hnext.gm0", "hnext.select", "hnext.scm1", "hnext.full"}
    if (case[2], case[3]) == br.E2E_SHAPE:
        want.add("e2e")
    assert want <= set(res), want - set(res)


def test_case_table_covers_what_it_claims():
    shapes = {(c[0], c[1]) for c in br.CASES}
    assert shapes == {(3, 86), (7, 86), (3, 256), (2, 401), (5, 101)}
    for C in (128, 256):
        mine = [c for c in br.CASES if c[2] == C]
        assert {(c[3], c[4]) for c in mine} == {(64, 64), (128, 100), (704, 682)}
        assert {c[5] for c in mine} == {"randn", "lowvar", "scaled"} and {c[6] for c in mine} == {True, False}
        assert any(c[7][0] == C for c in mine)
    assert any(c[2] == 256 and c[7] == (704, 682) for c in br.CASES)
    # (7, 86): stripe 1 uses all four modulation slots, stripe 2 clamps at the last batch row; (3, 86): a stripe of two rows
    _, _, b, slot = br.row_map(602, 86)
    assert sorted(set(slot[256:512].tolist())) == [0, 1, 2, 3] and int(b[256]) == 2 and int(b[-1]) == 6 == (602 - 1) // 86
    assert 258 - br.STRIPE == 2 and all(n >= br.MIN_TOKENS for _, n in shapes)


def _bad(blk, case, defect, names):
    """Out-of-bound counts of the named checks with ``defect`` injected into the emulation."""
    ops, clean = _case(blk, case)
    assert all(c.nbad == 0 for c in clean.values())
    res = br.check_case(ops, lambda o, la: br.emulate(o, la, defect), out=lambda s: None)
    counts = {n: res[n].nbad for n in names}
    print(f"DEFECT {defect} {br.case_id(blk, case)} {counts}")
    return counts


def _find(B, N, C):
    for c in br.CASES:
        if (c[0], c[1], c[2]) == (B, N, C):
            return c
    raise KeyError((B, N, C))


@pytest.mark.parametrize("C", [128, 256])
def test_defect_01_stripe_last_row_reads_the_next_batch_rows_ga(C):          # caught by: x1
    n = _bad(1, _find(7, 86, C), "ga_next_row", ["x1"])
    assert n["x1"] > C                   # rows 255 and 511 read the wrong vector: more than half of their 2 C elements must leave the bound
    assert _bad(2, _find(7, 86, C), "ga_next_row", ["probe"])["probe"] >= C


@pytest.mark.parametrize("blk,C", [(1, 128), (2, 256)])
def test_defect_02_eps_and_eps_next_swapped(blk, C):                          # caught by: select and hnext
    case = _find(7, 86, C)
    n = _bad(blk, case, "eps_swapped", ["select", "hnext.select", "hnext.gm0"])
    M = 602 * C
    assert n["select"] > 0.05 * M and n["hnext.select"] > 0.05 * M and n["hnext.gm0"] > 0.05 * M


@pytest.mark.parametrize("blk,C", [(1, 256), (2, 128)])
def test_defect_03_sn_and_hs_swapped(blk, C):                                 # caught by: hnext
    n = _bad(blk, _find(3, 86, C), "sn_hs_swapped", ["hnext.full", "select"])
    assert n["hnext.full"] > 0.5 * 258 * C and n["select"] == 0


@pytest.mark.parametrize("blk,C", [(1, 128), (2, 256)])
def test_defect_04_layernorm_statistics_from_the_unrounded_x1(blk, C):        # caught by: select
    assert _bad(blk, _find(3, 86, C), "stats_unrounded", ["select"])["select"] > 0


@pytest.mark.parametrize("C", [128, 256])
def test_defect_05_rounding_of_ga_yin_skipped(C):                             # caught by: x1
    assert _bad(1, _find(3, 86, C), "gy_unrounded", ["x1"])["x1"] > 0.005 * 258 * C
    assert _bad(2, _find(3, 86, C), "gy_unrounded", ["probe"])["probe"] > 0.005 * 258 * C


@pytest.mark.parametrize("blk,C", [(1, 256), (2, 128)])
def test_defect_06_one_xor_lane_step_missing_in_the_mean(blk, C):             # caught by: select
    assert _bad(blk, _find(2, 401, C), "mean_lane_step", ["select"])["select"] > 0.3 * 802 * C


@pytest.mark.parametrize("blk,C", [(1, 128), (2, 256)])
def test_defect_07_modulation_slot_3_aliased_to_slot_2(blk, C):               # caught by: x1 (ga), select (sc, sh, gm), hnext (sn, hs)
    first = "x1" if blk == 1 else "probe"
    n = _bad(blk, _find(7, 86, C), "slot3_alias", [first, "select", "hnext.full"])
    rows = int((br.row_map(602, 86)[3] == 3).sum())
    assert rows == 512 - 5 * 86 and all(v > 0.5 * rows * C for v in n.values())
    # a shape without a fourth slot cannot see it
    assert sum(_bad(blk, _find(3, 256, C), "slot3_alias", [first, "select"]).values()) == 0


@pytest.mark.parametrize("blk,C", [(1, 128), (2, 128), (1, 256), (2, 256)])
def test_defect_08_a_tile_group_visited_twice_under_rotation(blk, C):         # caught by: select (and scm1)
    case = _find(7, 86, C)
    n = _bad(blk, case, "tile_group_twice", ["select", "scm1"])
    assert n["select"] > 0 and n["scm1"] > 0
    ops = _case(blk, case)[0]
    assert ops["launches"]["select"]["mlp"][4] // 64 >= 2       # the select launch has more than one rotation group


@pytest.mark.parametrize("C", [128, 256])
def test_defect_09_gate_column_k_mod_32(C):                                   # caught by: probe (bit-exact) and x1(W_o)
    n = _bad(2, _find(3, 86, C), "gate_col_mod32", ["probe", "x1(W_o)"])
    assert n["probe"] > 0.2 * 258 * C and n["x1(W_o)"] > 0


@pytest.mark.parametrize("C", [128, 256])
def test_defect_10_out_projection_bias_dropped(C):                            # caught by: x1(W_o) (the probe has b_o = 0 and cannot)
    n = _bad(2, _find(3, 86, C), "bo_dropped", ["x1(W_o)", "probe"])
    assert n["x1(W_o)"] > 0.2 * 258 * C and n["probe"] == 0
    # lowvar scales b_o by 2^-9 along with the activations of every third row: still seen
    assert _bad(2, _find(7, 86, C), "bo_dropped", ["x1(W_o)"])["x1(W_o)"] > 0


def test_defect_11_w_o_chunk_3_taken_from_chunk_0():                          # caught by: probe and x1(W_o), C = 256 only (WO_CHUNKS == 4)
    n = _bad(2, _find(3, 86, 256), "wo_chunk3_from_0", ["probe", "x1(W_o)"])
    assert n["probe"] > 0.2 * 258 * 256 and n["x1(W_o)"] > 0.2 * 258 * 256


@pytest.mark.parametrize("C", [128, 256])
def test_defect_12_epilogue_x1_recomputed_from_the_parked_tok(C):             # caught by: x1(W_o) and probe (gm = 0: tok must BE x1)
    n = _bad(2, _find(5, 101, C), "x1_from_parked_tok", ["x1(W_o)", "probe"])
    assert n["probe"] > 0.3 * 505 * C and n["x1(W_o)"] > 0.3 * 505 * C


def test_lowvar_makes_an_eps_mix_up_a_gross_error():
    """The class does what it is for: with eps comparable to the variance the swapped eps moves far more elements of h."""
    C = 128
    low = _bad(1, _find(7, 86, C), "eps_swapped", ["select"])["select"] / (602 * C)
    plain = _bad(1, _find(3, 86, C), "eps_swapped", ["select"])["select"] / (258 * C)
    assert low > 2 * plain, (low, plain)
