"""CPU: the references, bounds and dispatch mirror of tests/head_step_reference.py, before a GPU sees them.

  * the numpy float64 references, teacher-forced on the pinned oracle's own float64 outputs, reproduce it to round-off (1e-12; the project's
    oracle-vs-reference figure is 5e-15): forward slots, grad_x0 / grad_theta, and the eleven GEMM gradients recomputed from D4 / DO;
  * a correct fp32 implementation (``emulate_forward`` / ``emulate_sweep``: plain left-to-right sums, the fp32 activation formulas, the
    hi / lo' split through np.float16 for the multi-path form) stays inside every bound, on every element, for every input class;
  * each injected defect leaves the bound on at least one element, at a short and at a long step count;
  * the activation error constants hold for the same formulas in float32 against float64;
  * ``route_forward`` / ``route_backward`` agree with every host-visible fact: the set of reachable instantiations, the case table of the
    GPU file, the workspace-size entry points and the dims the host refuses.

Defects and where the bound sees them (every one at a short AND at a long step count, in every family it applies to).  Forward, one
step, so the step count does not enter the bound: the dropped hi lo' cross term and the flushed f16-subnormal weight (the historical
defect; class ``sub``) in the multi-path form, one omitted reduction index, h_{t-1} of the wrong layer (two layers and more; T >= 2,
at T = 1 every h_{t-1} is zero), c_n used without its bias.  Sweep: the dropped carry u dh (T >= 2: one step carries nothing), the
ignored clamp rule (class ``clamp``), one omitted reduction index, and again the dropped cross term and the flushed subnormal weight:
at hidden 64 one step's worst-case depth is D_STEP = 423 roundings (2.5e-5 of the magnitude sum), which hides a 2^-12 defect in the
elements whose 192 terms cancel little, but not in all of them -- D4 leaves its bound by a factor of 3 to 100.  No bound was scaled to
make a defect show.  The multi-path SWEEP defects run on family ``mp`` (two layers) only: ``mp_bwd_applicable`` admits L = 2 alone, a
one-layer head's sweep runs the fp32 v2 kernels whatever the forward ran, so ``mp-L1`` has forward defects and no sweep defects.  For the
dropped cross term and the flushed subnormal weight in the sweep only D4 leaves its bound (DO, grad_x0, grad_theta stay below 0.35 of
theirs: grad_x0 / grad_theta carry the whole chain's depth, DO of the last step has no split product behind it).
"""
import numpy as np
import pytest

import head_step_reference as R

F4, F8 = np.float32, np.float64
FAMILIES = {"fp32": dict(S=2, H=24, L=2, P=3, mp=False), "fp32-L3": dict(S=3, H=20, L=3, P=1, mp=False),
            "mp": dict(S=2, H=64, L=2, P=3, mp=True), "mp-L1": dict(S=1, H=64, L=1, P=3, mp=True)}


def _case(family, T, kind="randn", B=3):
    f = FAMILIES[family]
    return dict(id=f"{family}-T{T}-{kind}", dims=(B, T, f["S"], f["P"], 8, f["H"], f["L"]), mp=-1, v1=False, kind=kind), f["mp"]


_FWD_CACHE = {}


def _forward(family, T, kind, fault=None):
    """(inputs, G, outputs of the fp32 emulation); computed once per key and never modified."""
    key = (family, T, kind, fault)
    if key not in _FWD_CACHE:
        # one step: more paths instead.  Class clamp: at hidden 64 the sweep's magnitude grows by a factor of 2 - 3 per step back in time,
        # so 17 steps from the end the bound no longer decides the clamp rule (every diagonal below the floor counts as ambiguous there);
        # the rule is decided in the last steps, and 8 paths make sure one of them has a zeroed diagonal there
        case, mp = _case(family, T, kind, B=16 if T == 1 else 8 if kind == "clamp" else 3)
        inp = R.make_inputs(case)
        G = R.project32(inp["ctx"], inp["ws"], case["dims"][2])
        out = R.emulate_forward(inp["ws"], inp["x0"], inp["theta"], inp["eps"], G, inp["dt"], mp=mp, fault=fault)
        for a in out:
            a.setflags(write=False)
        _FWD_CACHE[key] = (inp, G, out, mp, case["dims"])
    return _FWD_CACHE[key]


def _score_forward(inp, G, out, mp):
    paths, means, chol, raw, acts = out
    ref = R.forward_ref(inp["ws"], inp["theta"], inp["eps"], G, paths, acts, inp["dt"], mp=mp)
    got = dict(acts=acts, means=means, chol_raw=raw, chol=chol, next=paths[:, 1:])
    return {k: R.excess(got[k], *ref[k]) for k in got}


def _score_sweep(inp, out, mp, dims, fault=None):
    paths, means, chol, raw, acts = out
    P = dims[3]
    got = R.emulate_sweep(inp["ws"], P, inp["eps"], raw, acts, inp["gp"], inp["gm"], inp["gl"], inp["dt"], mp=mp, fault=fault)
    ref, _ = R.sweep_ref(inp["ws"], P, inp["eps"], raw, acts, inp["gp"], inp["gm"], inp["gl"], inp["dt"], mp=mp)
    return {k: R.excess(g, *ref[k]) for k, g in zip(("D4", "DO", "grad_x0", "grad_theta"), got)}


# ------------------------------------------------------------------------------------------------- activation constants
def test_activation_error_terms_cover_the_fp32_formulas():
    """E_sig / E_tanh against the same formulas evaluated in float32 (numpy's exp2 and division are within the 1 ulp the ISA
    documents for v_exp_f32 / v_rcp_f32): 400,000 arguments in [-45, 45] and the saturated tails; worst ratio printed."""
    g = np.random.default_rng(5)
    x = np.concatenate([g.uniform(-45, 45, 200000), g.standard_normal(200000) * 3, [-100.0, -88.0, -30.0, 0.0, 30.0, 88.0, 100.0]]).astype(F4)
    x8 = x.astype(F8)
    rs = np.abs(R.sigmoid32(x).astype(F8) - R.sig64(x8)) / (R.e_sig(x8) + R.FLOOR)
    rt = np.abs(R.tanh32(x).astype(F8) - np.tanh(x8)) / (R.e_tanh(x8) + R.FLOOR)
    print(f"sigmoid worst err/bound {rs.max():.3g}, tanh {rt.max():.3g}")
    assert rs.max() <= 1 and rt.max() <= 1
    assert float(R.e_sig(x8).max()) <= 2 * R.ULP_T * 1.0001


# ------------------------------------------------------------------------------------------------- anchoring to the oracle
@pytest.mark.parametrize("dims", [(4, 9, 2, 3, 8, 20, 2), (3, 5, 3, 1, 6, 12, 3), (2, 1, 1, 2, 4, 16, 1)], ids=["L2", "L3", "L1-T1"])
def test_references_reproduce_the_oracle_in_float64(dims):
    from oracle import vsde_oracle as vo
    B, T, S, P, C, H, L = dims
    dt, dm = 0.25, 2.0 ** -6                      # dt, sqrt(dt), diag_min exact in float32: the references round them as the kernels do
    inp = R.make_inputs(dict(dims=dims, kind="randn"), seed=3)
    inp["ws"][8][S] *= F4(0.05)                    # first diagonal around the floor: it binds on part of the steps
    inp["ws"][9][S] = F4(dm)
    w64 = [a.astype(F8) for a in inp["ws"]]
    x0, ctx, theta, eps = (inp[k].astype(F8) for k in ("x0", "ctx", "theta", "eps"))
    gp, gm, gl = (inp[k].astype(F8) for k in ("gp", "gm", "gl"))
    w = vo.HeadWeights(*w64)
    f = vo.head_forward(x0, ctx, theta, eps, w, dt, True, np.float64, dm)
    g = vo.head_backward(gp, gm, gl, ctx, theta, eps, f, w, dt, np.float64, dm)
    diag = f.chol_raw[..., [i * (i + 1) // 2 + i for i in range(S)]]
    assert T == 1 or ((diag < dm).any() and (diag >= dm).any())
    G = ctx @ w64[0][:, S:S + C].T + w64[2]
    ref = R.forward_ref(w64, theta, eps, G, f.paths, f.acts, dt, diag_min=dm)
    for name, got in (("acts", f.acts), ("means", f.means), ("chol_raw", f.chol_raw), ("chol", f.chol), ("next", f.paths[:, 1:])):
        assert np.abs(ref[name][0] - got).max() <= 1e-12, name
    assert np.array_equal(R.chol_identities(f.chol, f.chol_raw, dm), f.chol)
    sw, _ = R.sweep_ref(w64, P, eps, f.chol_raw, f.acts, gp, gm, gl, dt, diag_min=dm)
    assert np.abs(sw["grad_x0"][0] - g.x0).max() <= 1e-12 and np.abs(sw["grad_theta"][0] - g.sde_parameters).max() <= 1e-12
    # the eleven GEMM gradients from the new D4 / DO
    D4, DO = sw["D4"][0], sw["DO"][0]
    pi = lambda l: np.concatenate([D4[:, :, l, 0], D4[:, :, l, 1], D4[:, :, l, 2]], -1)
    ph = lambda l: np.concatenate([D4[:, :, l, 0], D4[:, :, l, 1], D4[:, :, l, 3]], -1)
    hprev = np.concatenate([np.zeros((B, 1, L, H)), f.acts[:, :-1, :, 0]], 1)
    x_in = np.concatenate([f.paths[:, :-1], ctx, np.broadcast_to(theta[:, None], (B, T, P))], -1)
    tn = lambda X, Y: np.einsum("btn,btk->nk", X, Y)
    want = [(g.context, pi(0) @ w64[0][:, S:S + C]), (g.W_ih_l0, tn(pi(0), x_in)), (g.W_hh_l0, tn(ph(0), hprev[:, :, 0])),
            (g.b_ih_l0, pi(0).sum((0, 1))), (g.b_hh_l0, ph(0).sum((0, 1))), (g.out_weight, tn(DO, f.acts[:, :, L - 1, 0])),
            (g.out_bias, DO.sum((0, 1)))]
    if L > 1:
        want += [(g.W_ih_stack, np.stack([tn(pi(l), f.acts[:, :, l - 1, 0]) for l in range(1, L)])),
                 (g.W_hh_stack, np.stack([tn(ph(l), hprev[:, :, l]) for l in range(1, L)])),
                 (g.b_ih_stack, np.stack([pi(l).sum((0, 1)) for l in range(1, L)])),
                 (g.b_hh_stack, np.stack([ph(l).sum((0, 1)) for l in range(1, L)]))]
    for a, b in want:
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, float(np.abs(a).max()))


# --------------------------------------------------------------------------------------- a correct implementation stays inside
INSIDE = [(fam, T, "randn") for fam in FAMILIES for T in (1, 2, 17)] + [(fam, 17, k) for fam in ("fp32", "mp") for k in R.KINDS[1:]] \
    + [("fp32", 33, "randn"), ("mp", 33, "randn")]


@pytest.mark.parametrize("family, T, kind", INSIDE, ids=[f"{f}-T{T}-{k}" for f, T, k in INSIDE])
def test_a_correct_fp32_implementation_stays_inside_every_bound(family, T, kind):
    inp, G, out, mp, dims = _forward(family, T, kind)
    fwd = _score_forward(inp, G, out, mp)
    bwd = _score_sweep(inp, out, mp, dims)
    print(" ".join(f"{k} {v[1]:.3g}" for k, v in {**fwd, **bwd}.items()))
    for k, (nbad, worst, where) in {**fwd, **bwd}.items():
        assert nbad == 0, (k, nbad, worst, where)
    assert np.array_equal(R.chol_identities(out[2], out[3]), out[2])
    if kind == "clamp":
        raw = out[3]
        below = float((raw[..., 0] < F4(R.DIAG_MIN)).mean())
        assert 0.1 <= below <= 0.9, below                               # the floor binds on a good part of the steps, not on all
        assert (raw[..., -1] == F4(R.DIAG_MIN)).all()                   # and one diagonal sits exactly on it


# --------------------------------------------------------------------------------------------- every defect leaves the bound
FWD_FAULTS = [("no_cross", "mp", "randn", (2, 17)), ("no_cross", "mp-L1", "randn", (1, 17)), ("flush_sub", "mp", "sub", (2, 17)),
              ("flush_sub", "mp-L1", "sub", (1, 17)), ("skip_index", "fp32", "randn", (2, 17)), ("skip_index", "fp32-L3", "randn", (2, 17)),
              ("skip_index", "mp", "randn", (2, 17)), ("skip_index", "mp-L1", "randn", (1, 17)), ("wrong_layer", "fp32", "randn", (2, 17)), ("wrong_layer", "fp32-L3", "randn", (2, 17)),
              ("wrong_layer", "mp", "randn", (2, 17)), ("cn_no_bias", "fp32", "randn", (1, 17)), ("cn_no_bias", "fp32-L3", "randn", (1, 17)),
              ("cn_no_bias", "mp", "randn", (1, 17)), ("cn_no_bias", "mp-L1", "randn", (1, 17))]
FWD_FAULT_CASES = [(f, fam, k, T) for f, fam, k, Ts in FWD_FAULTS for T in Ts]


@pytest.mark.parametrize("fault, family, kind, T", FWD_FAULT_CASES, ids=[f"{f}-{fam}-T{T}" for f, fam, k, T in FWD_FAULT_CASES])
def test_every_forward_defect_leaves_the_bound(fault, family, kind, T):
    inp, G, out, mp, dims = _forward(family, T, kind, fault)
    res = _score_forward(inp, G, out, mp)
    nbad = sum(v[0] for v in res.values())
    print(fault, {k: (v[0], round(v[1], 2)) for k, v in res.items()})
    assert nbad > 0, "the defect stayed inside the bound"


SWEEP_FAULT_LIST = [("no_cross", "mp", "randn", (2, 17)), ("flush_sub", "mp", "sub", (2, 17)), ("drop_carry", "fp32", "randn", (2, 17)), ("drop_carry", "fp32-L3", "randn", (2, 17)), ("drop_carry", "mp", "randn", (2, 17)),
                    ("ignore_clamp", "fp32", "clamp", (1, 17)), ("ignore_clamp", "fp32-L3", "clamp", (1, 17)), ("ignore_clamp", "mp", "clamp", (1, 17)),
                    ("skip_index", "fp32", "randn", (2, 17)), ("skip_index", "fp32-L3", "randn", (2, 17)), ("skip_index", "mp", "randn", (2, 17))]
SWEEP_FAULT_CASES = [(f, fam, k, T) for f, fam, k, Ts in SWEEP_FAULT_LIST for T in Ts]


@pytest.mark.parametrize("fault, family, kind, T", SWEEP_FAULT_CASES, ids=[f"{f}-{fam}-T{T}" for f, fam, k, T in SWEEP_FAULT_CASES])
def test_every_sweep_defect_leaves_the_bound(fault, family, kind, T):
    inp, G, out, mp, dims = _forward(family, T, kind)
    res = _score_sweep(inp, out, mp, dims, fault)
    print(fault, {k: (v[0], round(v[1], 2)) for k, v in res.items()})
    assert sum(v[0] for v in res.values()) > 0, "the defect stayed inside the bound"


def test_defect_lists_cover_the_issue():
    assert {f for f, *_ in FWD_FAULTS} == set(R.FORWARD_FAULTS)
    assert {f for f, *_ in SWEEP_FAULT_LIST} == set(R.SWEEP_FAULTS)


# ------------------------------------------------------------------------------------------------------ dispatch mirror
def _sweep_routes():
    fw, bw = set(), set()
    for H in list(range(1, 65)) + [65, 80, 130, 1024]:
        for S in list(range(1, 12)) + [32]:
            for L in (1, 2, 3, 4):
                for B in (3, 31, 32, 512, 513, 1024, 1025, 2048, 2049):
                    d = (B, 2, S, 3, 16, H, L)
                    if R.check_dims(d):
                        continue
                    for mode in (-1, 0, 1, 2, 4, 8, 16):
                        for v1 in (False, True):
                            fw.update(R.route_forward(d, s, mode, v1) for s in (True, False))
                            bw.add(R.route_backward(d, mode, v1))
    return fw, bw


def test_kernel_lists_are_what_the_mirror_can_reach_and_the_case_table_reaches_all_of_them():
    fw, bw = _sweep_routes()
    assert sorted(fw) == list(R.FORWARD_KERNELS) and sorted(bw) == list(R.BACKWARD_KERNELS)
    assert len(R.FORWARD_KERNELS) == 59 and len(R.BACKWARD_KERNELS) == 29
    cfw, cbw = set(), set()
    for c in R.CASES:
        assert R.check_dims(c["dims"]) is None and c["kind"] in R.KINDS
        B, T, S, P, C, H, L = c["dims"]
        assert (B <= 40 or (T == 2 and c["id"] == "v1-L3-B300-T2")) and C <= 16
        if c["v1"]:
            assert H <= 64 and R.n_out(S) <= 64              # the guard in front of the v1 kernels
        if c["mp"] > 0:
            assert R.mp_applicable(H, L, S) and c["mp"] in (2, 4, 8, 16)
        cfw.update(R.route_forward(c["dims"], s, c["mp"], c["v1"]) for s in (True, False))
        cbw.add(R.route_backward(c["dims"], c["mp"], c["v1"]))
    assert sorted(cfw) == list(R.FORWARD_KERNELS), sorted(set(R.FORWARD_KERNELS) - cfw)
    assert sorted(cbw) == list(R.BACKWARD_KERNELS), sorted(set(R.BACKWARD_KERNELS) - cbw)
    assert len({c["id"] for c in R.CASES}) == len(R.CASES)
    ts = lambda pre: {c["dims"][1] for c in R.CASES if c["id"].startswith(pre)}
    assert set(R.T_SET) <= ts("v2") and {1, 2, 3, 17, 33} <= ts("mp")
    assert R.v1_wpb((300, 2, 2, 3, 16, 64, 3)) == 2 and R.v1_wpb((300, 2, 2, 3, 16, 64, 3), True) == 2 and R.v1_wpb((3, 2, 2, 3, 16, 64, 3)) == 1
    assert {R.wide_block(c["dims"]) for c in R.CASES if c["id"].startswith("wide")} >= {128, 192}
    assert R.route_forward((31, 17, 2, 3, 16, 64, 2), True).startswith("head_fwd_v2") and R.route_backward((31, 17, 2, 3, 16, 64, 2)).startswith("head_bwd_v2")
    assert R.route_forward((32, 17, 2, 3, 16, 64, 2), True) == "head_fwd_mp_kernel<2, true, 2, 2, 1>"
    assert R.route_backward((32, 17, 2, 3, 16, 64, 2)) == "head_bwd_mps_kernel<2, 2>"
    # the one CH = 8 forward launch: fwd_v2_lds beyond 80 KB in the training launch only
    assert R.fwd_v2_lds(64, 5, 2, 16, True) * 4 > 80 * 1024 >= R.fwd_v2_lds(64, 5, 2, 16, False) * 4
    assert R.fwd_v2_lds(64, 4, 2, 16, True) * 4 <= 80 * 1024 and R.fwd_v2_lds(64, 9, 1, 16, True) * 4 <= 80 * 1024


def test_mirror_agrees_with_the_host_entry_points():
    """Without a GPU the host shows: which dims it refuses (a workspace size of 0), where the forward workspace carries the multi-path
    fragment block (mp_applicable) and where the backward one does (mp_bwd_applicable)."""
    import ctypes
    import head_gemm_reference as RG
    from viforsdes_amd import _hip
    lib = _hip.load()
    fake = ctypes.c_void_p(4096)                 # never dereferenced: check_dims and the workspace check come before any HIP call
    w, view = _hip._Weights(*[fake] * 10), _hip._CtxView(fake, 0, 17 * 16, 16)
    code = lambda d: lib.vsde_debug_head_context_projection(ctypes.byref(_hip._Dims(*d)), ctypes.byref(view), ctypes.byref(w), fake, fake,
                                                            ctypes.c_size_t(0), None)
    for d in [(4, 16, 2, 3, 16, 64, 5), (4, 16, 2, 3, 16, 64, 0), (4, 16, 2, 3, 16, 1025, 1), (4, 16, 33, 3, 16, 64, 1), (0, 16, 2, 3, 16, 64, 1),
              (4, 16, 32, 3, 16, 1024, 4), (4, 16, 2, 3, 16, 1024, 4), (4, 16, 32, 3, 16, 64, 2), (4, 16, 10, 3, 16, 130, 1)]:
        refused = R.check_dims(d) is not None
        assert code(d) == R.ERROR_CODES[R.check_dims(d) or "VSDE_E_WORKSPACE"], d      # admitted dims: the empty workspace is what is refused
        assert (_hip.head_forward_workspace_bytes(*d) == 0) == refused, d
        assert (_hip.head_backward_workspace_bytes(*d) == 0) == refused, d
    a256 = lambda n: (n + 255) & ~255
    frag = lambda L, S: a256(((2 * L - 1) * 3072 + ((R.n_out(S) + 3) // 4) * 256) * 16)       # mp_frag_bytes, vsde_head_mp.hip:1261-1264
    for H in (32, 64, 80):
        for L in (1, 2, 3):
            base = _hip.head_forward_workspace_bytes(4, 16, 3, 3, 16, H, L)                    # S = 3: never multi-path
            for S in (1, 2, 4):
                want = base + a256(256 * R.n_out(S)) - a256(256 * R.n_out(3)) + (frag(L, S) if R.mp_applicable(H, L, S) else 0)
                assert _hip.head_forward_workspace_bytes(4, 16, S, 3, 16, H, L) == want, (H, L, S)
                d = (4, 16, S, 3, 16, H, L)
                extra = _hip.head_backward_workspace_bytes(*d) - RG.backward_workspace_bytes(d, 0)
                assert (extra > 0) == R.mp_bwd_applicable(H, L, S) and extra >= 0, d
