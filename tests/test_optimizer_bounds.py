"""CPU: the bounds of tests/optimizer_reference.py are sound and sensitive.

* ``step64`` equals clip_grad_norm_ + torch.optim.AdamW (not fused) + torch.lerp in float64 to 1e-12 of the magnitude;
* the constants of the module are at least 4 x the ratios of ``step32`` re-measured here over every case of
  tests/test_optimizer_ops_gpu.py -- so ``step32`` passes every bound;
* each of the 16 injected defects is rejected by the bounds on at least one class (the class is printed);
* the integer bf16 cast equals ``torch.Tensor.to(torch.bfloat16)`` bit for bit over every pattern class of the pack test."""
import numpy as np
import pytest
import torch

import optimizer_reference as R


def test_step64_equals_float64_torch():
    """5 steps on a two-group toy; gradient norms alternate between far below and far above max_norm = 1."""
    rng = np.random.default_rng(3)
    sizes, gids = [7, 33, 5], [0, 0, 1]
    groups = R.GROUPS[[0, 2]]
    params = [torch.nn.Parameter(torch.tensor(rng.standard_normal(n))) for n in sizes]
    opt = torch.optim.AdamW([dict(params=[q for q, gi in zip(params, gids) if gi == k], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
                             for k, (lr, b1, b2, eps, wd) in enumerate(groups)], foreach=False, fused=False)
    shadow = [q.detach().clone() + 0.01 for q in params]
    cat = lambda ts: np.concatenate([t.detach().numpy().ravel() for t in ts])
    state = {"p": cat(params), "m": np.zeros(sum(sizes)), "v": np.zeros(sum(sizes)), "sh": cat(shadow)}
    for t in range(5):
        g = rng.standard_normal(sum(sizes)) * (10.0 if t % 2 else 0.01)
        c = dict(state, g=g, sizes=np.array(sizes), gid=np.repeat(gids, sizes), groups=groups, t=float(t), scale=None, max_norm=1.0,
                 ema_w=R.EMA_W)
        ref = R.step64(c)
        for q, gq in zip(params, np.split(g, np.cumsum(sizes)[:-1])):
            q.grad = torch.tensor(gq)
        norm = torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        with torch.no_grad():
            for s, q in zip(shadow, params):
                s.copy_(torch.lerp(s, q.detach(), R.EMA_W))
        want = {"p": cat(params), "m": cat([opt.state[q]["exp_avg"] for q in params]),
                "v": cat([opt.state[q]["exp_avg_sq"] for q in params]), "sh": cat(shadow), "norm": float(norm)}
        for k, w in want.items():
            assert R.ratio(ref[k], w, ref["mag"][k]) * R.C24 <= 1e-12, (t, k)
        assert ref["t_next"] == float(opt.state[params[0]]["step"]) == t + 1 and not ref["found_inf"]
        state = {k: ref[k] for k in ("p", "m", "v", "sh")}


def test_a_found_inf_under_a_scale_skips_the_step_and_still_lerps():
    c = R.make_case("general", [9], [0], t=9, scale=1024.0)
    c["g"][3] = np.inf
    ref = R.step64(c)
    assert ref["found_inf"] and ref["t_next"] == 9.0
    for k in ("p", "m", "v"):
        assert np.array_equal(ref[k], c[k].astype(np.float64)) and not ref["mag"][k].any()
    sh, p = c["sh"].astype(np.float64), c["p"].astype(np.float64)
    assert np.array_equal(ref["sh"], sh + R.EMA_W * (p - sh))
    got = R.step32(c)
    assert got["found_inf"] and R.within({k: v for k, v in R.ratios(c, got, ref).items() if k != "norm"})


def test_constants_are_four_times_the_float32_ratios_at_every_gpu_case():
    worst = dict.fromkeys(R.KINDS, 0.0)
    for name, make in R.all_gpu_cases():
        c = make()
        ref = R.step64(c)
        r = R.ratios(c, R.step32(c), ref)
        assert R.within(r), (name, r)
        r["norm"] = R.ratio(R.step32(c, norm_order="sequential")["norm"], ref["norm"], ref["mag"]["norm"])
        worst = {k: max(w, r.get(k, 0.0)) for k, w in worst.items()}
    print("step32 against step64, worst ratio per kind: " + ", ".join(f"{k} {w:.2f}" for k, w in worst.items()))
    for k, w in worst.items():
        assert 4 * w <= R.C[k], (k, w)


def defect_cases():
    """A cut through the full cross on the mixed table: every class under four (scale, max_norm, t) settings."""
    for cls in R.CLASSES:
        modes = R.max_norm_modes(cls)
        for i, (scale, t) in enumerate(((1024.0, 0), (None, 9), (2.0 ** -10, 999), (None, 100000), (1024.0, 1))):
            mode = modes[(i + 1) % len(modes)]
            yield f"{cls} (scale {scale}, max_norm {mode}, t {t})", R.make_case(cls, R.MIXED_SIZES, R.MIXED_GIDS, t=t, scale=scale, mode=mode)


@pytest.fixture(scope="module")
def scored_cases():
    return [(name, c, R.step64(c)) for name, c in defect_cases()]


def test_step32_passes_on_the_defect_cases(scored_cases):
    for name, c, ref in scored_cases:
        assert R.within(R.ratios(c, R.step32(c), ref)), name


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_defect_is_rejected(defect, scored_cases):
    rejected = [name for name, c, ref in scored_cases if not R.within(R.ratios(c, R.step32(c, defect), ref))]
    print(f"defect {defect}: rejected on {len(rejected)} of {len(scored_cases)} cases, first on {rejected[0] if rejected else None}; "
          f"classes: {sorted({r.split(' ')[0] for r in rejected})}")
    assert rejected, defect


def test_integer_bf16_cast_equals_the_torch_cast():
    for name, u in list(R.pack_patterns().items()) + [("randn", R.pack_values())]:
        want = torch.from_numpy(u.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
        got = R.bf16_rne_bits(u)
        nan = R.bf16_is_nan(want)
        assert np.array_equal(R.bf16_is_nan(got), nan), name                       # a NaN stays a NaN; the payload is free
        assert np.array_equal(got[~nan], want[~nan]), name
        if name == "nan":
            assert nan.all()
        elif name != "randn":
            assert not nan.any()


def test_the_pattern_classes_are_what_their_names_say():
    pats = R.pack_patterns()
    cast = lambda k: R.bf16_rne_bits(pats[k])
    up = lambda k: (pats[k] >> 16).astype(np.uint16)
    assert np.array_equal(cast("tie_even"), up("tie_even")) and np.array_equal(cast("tie_odd"), up("tie_odd") + 1)
    assert (pats["tie_even"] & 0x1FFFF == 0x08000).all() and (pats["tie_odd"] & 0x1FFFF == 0x18000).all()
    assert np.array_equal(cast("tie_plus_ulp"), up("tie_plus_ulp") + 1) and np.array_equal(cast("tie_minus_ulp"), up("tie_minus_ulp"))
    assert (cast("to_bf16_max") & 0x7FFF == 0x7F7F).all() and (cast("to_inf") & 0x7FFF == 0x7F80).all()
    assert list(cast("zero")) == [0x0000, 0x8000] and list(cast("inf")) == [0x7F80, 0xFF80]
    assert (cast("subnormal") & 0x7FFF <= 0x0080).all() and (cast("small_normal") & 0x7F80 != 0).all()
    assert 0x0080 in cast("subnormal") and 0x0000 in cast("subnormal") and 0x0001 in cast("subnormal")
    assert (cast("mantissa_ones")[:2] == [0x3F80, 0x4000]).all()
    assert R.PACK_SENTINEL not in cast("nan") and R.PACK_SENTINEL not in up("nan")
