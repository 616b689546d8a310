"""CPU: the inputs of the particle-filter sweep (tests/filter_sweep_reference.py), checked on the reference alone
so that tests/test_filter_sweep_gpu.py compares the kernels with something decidable.

* the dispatch mirror: ``ALL`` has 252 / 186 / 186 instantiations, every one has exactly one generated case, and the mirror names
  that instantiation for the case's call; its ``max_n`` is ``_hip.particle_filter_max_particles``; the refusals of the host;
* every generated network passes ``ReactionNetworkSDE`` validation and ``kernel_compatible()``, changes every species and has the
  reaction count of its bin;
* per case, the torch route in float64 under the case's key: every observation of the filters before the last has a particle ESS
  above N / 20; the last filter (positive dims started at 1e-3 of their scale) hits the 1e-6 floor; at most 2 resampling entries
  are undecidable (the float64 threshold within 1e-5 C_{N-1} of a cumulative sum), and at most 1e-3 of the entries of the sweep;
* per case, the first two segments of the torch route in fp32 against float64 from the same float64 starts under one key: within
  half of the propagation bound (1e-4 of the largest magnitude), so a kernel that misses 2e-4 is not excused by the model;
* the kept-states restatement of the guided and residual segments equals the two reference modules it restates."""
import numpy as np
import pytest
import torch

import filter_sweep_reference as fs
import guided_filter_reference as gref
import reaction_networks as rn
import residual_bridge_reference as rref

CASES = fs.cases()
LARGE = fs.large_cases()
_RES = {}


def _reference(case):
    if case.name not in _RES:
        res = fs.torch_filter(case)
        _RES[case.name] = (res, fs.reference_conditions(case, res))
    return _RES[case.name]


# -------------------------------------------------------------------------------------------------------------- dispatch mirror
def test_every_instantiation_has_exactly_one_case_and_the_mirror_names_it():
    assert [len(fs.ALL[op]) for op in fs.OPS] == [252, 186, 186]
    assert all(len(set(fs.ALL[op])) == len(fs.ALL[op]) for op in fs.OPS)
    named = [fs.instantiation(*c.call("filter")) for c in CASES]
    assert [n[:7] for n in named] == fs.ALL["filter"] == [c.elem for c in CASES]
    for op in ("replay", "anchored"):
        got = [fs.instantiation(*c.call(op))[:7] for c in CASES if c.count is None]
        assert sorted(got) == sorted(fs.ALL[op]) and len(set(got)) == len(got)
        assert all(isinstance(fs.instantiation(*c.call(op)[:7], True), str) for c in CASES[:3])       # no count form of a replay
    assert len(set(c.name for c in CASES + LARGE)) == len(CASES) + len(LARGE)
    assert 20 <= len(LARGE) <= 25 and all(c.elem in fs.ALL["filter"] for c in LARGE)
    # the instantiations whose dynamic LDS passes 64 KiB (pf_launch's attribute path): N ((S | 1) + 1) 4 + 1152 bytes, only at
    # S = 14, 15 (N = 1024) and S = 16 (N >= 896): the large cells run all six functions (Gaussian and count) at N = 1024
    over = {(n, s) for n in range(64, 1025, 64) for s in range(1, 17) if (n * ((s | 1) + 1) + 16 * 18) * 4 > 64 * 1024}
    assert over == {(1024, 14), (1024, 15), (896, 16), (960, 16), (1024, 16)}
    assert sum(c.elem[0] == 3 and c.elem[1] >= 14 and c.N == 1024 for c in LARGE) == 6


def test_max_n_of_the_mirror_is_the_bindings():
    from viforsdes_amd import _hip
    for c in CASES + LARGE:
        out = fs.instantiation(*c.call("filter"))
        assert out[7] == _hip.particle_filter_max_particles(c.kind, c.sde.state_dim, proposal=c.proposal), c.name
    assert all(c.N == fs.instantiation(*c.call("filter"))[7] for c in LARGE)
    assert {c.N for c in LARGE} == {512, 1024}


def test_the_mirror_refuses_what_the_host_refuses():
    f = fs.instantiation
    assert isinstance(f("filter", 3, 17, 0, False, "bootstrap", 2, False), str)
    assert isinstance(f("filter", 3, 5, 0, False, "bridge", 2, False), str)
    assert isinstance(f("filter", 3, 3, 0, False, "bridge", 5, False), str)
    assert isinstance(f("filter", 3, 3, 0, False, "bootstrap", 17, False), str)
    assert isinstance(f("filter", 4, 9, 3, False, "bootstrap", 2, False), str)
    assert isinstance(f("filter", 4, 3, 17, False, "bootstrap", 2, False), str)
    assert isinstance(f("filter", 1, 2, 0, False, "bootstrap", 2, False), str)
    assert isinstance(f("filter", 2, 2, 0, False, "bridge", 2, True), str)
    assert f("filter", 4, 8, 9, True, "bootstrap", 8, True) == (4, 8, 16, True, 0, True, False, 512)
    assert f("anchored", 4, 4, 4, False, "residual_bridge", 3, False) == (4, 4, 4, False, 4, False, True, 512)
    assert f("replay", 3, 3, 0, False, "residual_bridge", 2, False) == (3, 3, 2, False, 2, False, True, 1024)
    assert len(fs.refusal_classes()) == (2 + 16 + 8) + 2 * (2 + 4 + 4)


# --------------------------------------------------------------------------------------------------------------------- networks
@pytest.mark.parametrize("kinetic", [False, True])
@pytest.mark.parametrize("NR", [4, 8, 16])
@pytest.mark.parametrize("S", range(1, 9))
def test_generated_networks_are_valid_and_kernel_compatible(S, NR, kinetic):
    from viforsdes_amd import ReactionNetworkSDE
    from viforsdes_amd.core.sde import builtin_sde_kind
    kw, theta, start = rn.sweep_network(S, NR, kinetic)
    sde = ReactionNetworkSDE(**kw)
    assert sde.kernel_compatible() and builtin_sde_kind(sde) == "reaction_network"
    assert (sde.state_dim, sde.num_reactions) == (S, {4: 3, 8: 7, 16: 12}[NR]) and sde.sde_param_dim == len(theta) and len(start) == S
    assert all(any(row[i] != 0 for row in sde.change) for i in range(S))                   # every species is changed
    assert any(sum(row) == 2 for row in sde.reactants) and any(sum(row) == 0 for row in sde.reactants)
    assert sde.plain == (not kinetic)
    if kinetic:
        laws = [law for law in sde.laws if law is not None]
        assert len(laws) == (2 if S > 1 else 1) and sde.laws[0][2] == 2
    x, th = torch.tensor([start], dtype=torch.float64), torch.tensor([theta], dtype=torch.float64)
    assert bool(torch.isfinite(sde.drift(x, th)).all()) and bool(torch.isfinite(sde.diffusion(x, th)).all())


def test_named_networks_fall_into_their_cells():
    used = [c for c in CASES if c.elem[0] == 4 and (c.elem[1], c.elem[2], c.elem[3]) in fs.NAMED and c.elem[4] == 0 and not c.elem[5]]
    assert len(used) == len(fs.NAMED) == 5
    for c in used:
        kw = fs.NAMED[(c.elem[1], c.elem[2], c.elem[3])][0]
        assert c.sde.reactants == tuple(tuple(r) for r in kw["reactants"]) and c.sde.kernel_compatible()
        assert fs.instantiation(*c.call("filter"))[:7] == c.elem


def test_cells_cover_the_observation_forms():
    guided = [c for c in CASES if c.elem[4]]
    assert all(c.values.shape[1] == 4 for c in guided if c.elem[4] == 4)
    assert any(c.values.shape[1] > c.sde.state_dim for c in guided)
    s1 = [c.values.shape[1] for c in guided if c.elem[4] == 2 and c.elem[1] == 1]
    assert set(s1) == {1, 2} and 0.3 <= s1.count(1) / len(s1) <= 0.7
    assert all(c.values.shape[1] == 2 for c in guided if c.elem[4] == 2 and c.elem[1] > 1)
    count = [c for c in CASES if c.elem[5]]
    assert len(count) == 66 and {c.count for c in count} == {"poisson", "negative_binomial"}
    for kind in ("poisson", "negative_binomial"):
        assert {c.H is None for c in count if c.count == kind} == {True, False}
    assert all(c.rows == fs.ROWS and tuple(c.theta.shape[:1]) == (fs.M,) and c.N == fs.N for c in CASES)
    assert all(bool((c.values >= 0).all()) and bool((c.values == c.values.round()).all()) for c in count)


# ----------------------------------------------------------------------------------------------------- the float64 reference
@pytest.mark.parametrize("case", CASES + LARGE, ids=lambda c: c.name)
def test_reference_conditions_hold_in_float64(case):
    res, cond = _reference(case)
    print(f"{case.name}: smallest float64 ESS {cond['ess']:.1f} of {case.N}, floor hit {cond['floor_hit']}, "
          f"{cond['undecidable']} of {cond['entries']} entries undecidable, nearest threshold {cond['near']:.1e} C")
    assert bool(torch.isfinite(res.particles).all())
    assert cond["ess"] > case.N / 20
    assert cond["floor_hit"] or not case.pos
    if case.N == fs.N:
        assert cond["undecidable"] <= 2
        assert cond["near"] > fs.KEY_MARGIN * fs.ANCESTOR_MARGIN          # the case's key: see filter_sweep_reference.SALTS


def test_undecidable_share_of_the_sweep():
    total = sum(_reference(c)[1]["undecidable"] for c in CASES)
    entries = sum(_reference(c)[1]["entries"] for c in CASES)
    print(f"{total} of {entries} resampling entries of the sweep are undecidable in float64")
    assert total <= 1e-3 * entries


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_fp32_torch_route_is_within_half_the_propagation_bound(case):
    from viforsdes_amd.inference import particle_filter as pf
    res, _ = _reference(case)
    S, B = case.sde.state_dim, case.M * case.N
    key = fs.key_tensor(case.key)
    paths = torch.arange(B, dtype=torch.int64)
    bridge, residual = case.proposal != "bootstrap", case.proposal == "residual_bridge"
    worst = 0.0
    for k in (1, 3):                                         # rows 0 -> 3 and 3 -> 10
        anc = res.ancestors[:, k - 1].long()
        start = torch.gather(res.particles[:, k - 1], 1, anc[..., None].expand(-1, -1, S)).reshape(B, S)
        ends = []
        for dtype in (torch.float64, torch.float32):
            theta = case.theta.to(dtype)
            th = theta[:, None, :].expand(-1, case.N, -1).reshape(B, -1)
            advance = pf._segment_propagator(case.sde, case.obs, case.like, theta, case.dt, case.pos, bridge, residual)
            ends.append(advance(start.to(dtype), th, case.rows[k - 1], k, case.rows[k], paths, key)[0].double())
        worst = max(worst, float((ends[1] - ends[0]).abs().max() / ends[0].abs().max()))
    print(f"{case.name}: fp32 torch route against float64 over two segments: {worst:.2e} of the largest magnitude")
    assert worst <= 0.5 * fs.PROPAGATION_BOUND


# ------------------------------------------------------------------------------------------------- the kept-states restatement
@pytest.mark.parametrize("index", [140, 147, 200, 251])
def test_segment_restates_the_guided_and_residual_references(index):
    case = CASES[index]
    assert case.proposal != "bootstrap"
    S, B, n = case.sde.state_dim, 16, 7
    g = np.random.default_rng(index)
    start = np.abs(case.x0[0].double().numpy())[None] * (1.0 + 0.05 * g.standard_normal((B, S)))
    theta, z = np.repeat(case.theta[:1].double().numpy(), B, axis=0), g.standard_normal((B, n, S))
    H = None if case.H is None else case.H.double().numpy()
    y = case.values[3].double().numpy()
    for dtype in (np.float64, np.float32):
        coef = gref.sde_coefficients(case.sde, dtype)
        if case.proposal == "bridge":
            x, lr = gref.guided_segment(coef, start, theta, z, y, H, case.variance, case.dt, case.pos, dtype)
        else:
            x, lr, _ = rref.residual_segment(coef, start, theta, z, y, H, case.variance, case.dt, case.pos, dtype)
        states, lr2 = fs.segment(case, start, theta, z, 3, dtype)
        assert states.shape == (B, n, S) and np.array_equal(states[:, -1], x) and np.array_equal(lr2, lr)
