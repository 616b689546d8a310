"""GPU: every instantiation of the particle-filter kernels (csrc/vsde_filter_kernels.h: pf_kernel, rp_kernel, ar_kernel) that the
host dispatch can launch -- 252 filter, 186 genealogy-replay and 186 record-replay functions -- on one generated case each
(tests/filter_sweep_reference.py), plus the cells of ``large_cells()`` at N = max_n.

One test per element of ``ALL["filter"]`` makes three launches and scores each stage in float64 on the kernel's own previous stage,
as tests/test_particle_filter_gpu.py, test_guided_filter_gpu.py, test_residual_bridge_gpu.py, test_count_likelihood_gpu.py,
test_particle_smoother_gpu.py and test_pmmh_paths_gpu.py do, with their bounds:

* the filter (``_hip.particle_filter`` with the Gaussian or the count term, ``_hip.guided_particle_filter(residual=...)``):
  propagation per segment against the float64 step of the matching reference from the kernel's particles gathered through the
  kernel's ancestors, 2e-4 of the largest magnitude; guided and residual log-weights within 4 E32 + 1e-5 max(1, largest finite |lw|),
  E32 the error of the same reference run in fp32 (test_guided_filter_gpu.py / test_residual_bridge_gpu.py: ``_lw_errors``);
  increments 1e-5 max(1, largest finite |lw|), ESS, mean, std 1e-4 relative in the forms of test_particle_filter_gpu.py; exactly:
  ``particles[:, 0] == x0``, positive dims >= float32(1e-6) with the floor hit in the last filter, ancestors in [0, N) that never
  decrease in j, a shared row leaves the gathered particles unchanged bit for bit; log_likelihood = sum of increments;
* ancestors, per entry: a kernel ancestor differs from float64 systematic resampling of the float64 weights of the kernel's
  particles only by exactly 1 and only where float64's threshold lies within 1e-5 C_{N-1} of a cumulative sum (the fp32 scalar bound:
  the scan and the threshold make fewer than 30 fp32 roundings); at N = 64 at most 2 such undecidable entries per case and 1e-3 of
  the sweep's (the caps of tests/test_filter_sweep_bounds.py, re-asserted on the device data); at N = max_n, where 2 N 1e-5 of the
  entries are undecidable by that definition, the rule of the files above: at most 1e-3 of the entries differ;
* the genealogy replay (``_hip.filter_replay`` / ``_hip.guided_filter_replay``) of that store with host-drawn final slots: the
  lineage exactly, every step of every segment against the same float64 segments (2e-4), endpoints against the stored particles;
* the record replay (``_hip.anchored_replay`` / ``_hip.guided_anchored_replay``) of records formed in numpy from the same store
  along those lineages (anchors, ``m N + slot`` noise paths, the filter's key per record): the paths against the same float64
  segments (2e-4); how many are bit-identical to the genealogy replay's is printed, not asserted (two kernels, compiled
  separately); one record is marked dead and comes back NaN.

A last test makes no launch: for every (kind, S, proposal) class N = max_n + 64 raises ValueError from each filter entry point.

Observed on the MI355X (worst error / bound per kernel family over the sweep and the large cells; observed values, never used to
set a bound):

    family      f. propagation  f. log-weight  f. increments         f. ESS        f. mean         f. std   rp. segments  rp. endpoints  record replay
    bootstrap           0.343              -          0.148          0.163          0.465          0.238          0.317          0.000          0.310
    count               0.265              -          0.171          0.658          0.543          0.480          0.239          0.000          0.239
    guided              0.026          0.088          0.068          0.003          0.002          0.186          0.018          0.000          0.002
    residual            0.030          0.089          0.067          0.004          0.003          0.217          0.007          0.000          0.006

1332 of 1332 record paths bit-identical to the genealogy replay's; 0 of 241920 resampling entries of the N = 64 cases undecidable on
the device data; 3 of 352512 ancestors differ from float64, all in the large cells (f.: the filter, rp.: the genealogy replay)."""
import numpy as np
import pytest
import torch

import filter_sweep_reference as fs
import particle_filter_reference as ref
from philox_reference import forecast_noise

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = fs.cases()
LARGE = fs.large_cases()

_WORST = {}      # (family, quantity) -> worst error / bound of this run
_UNDECIDABLE = {}    # case name -> (undecidable entries, entries) on the device data


def _note(case, quantity, ratio):
    family = "count" if case.count else {"bootstrap": "bootstrap", "bridge": "guided", "residual_bridge": "residual"}[case.proposal]
    _WORST[(family, quantity)] = max(_WORST.get((family, quantity), 0.0), float(ratio))


def _device_inputs(case):
    from viforsdes_amd.core.sde import builtin_sde_route, kernel_theta
    kind, network = builtin_sde_route(case.sde)
    assert kind == case.kind
    d = lambda t: None if t is None else t.to(DEV)
    rows = torch.tensor(case.rows, dtype=torch.int32, device=DEV)
    values = d(case.values)
    term = case.variance if case.count is None else case.like.kernel_terms(values)
    return dict(kind=kind, network=network, x0=d(case.x0), theta=kernel_theta(network, d(case.theta)), rows=rows, values=values,
                H=d(case.H), term=term, key=fs.key_tensor(case.key).to(DEV))


def _filter(case, a, N=None):
    from viforsdes_amd import _hip
    N = case.N if N is None else N
    if case.proposal == "bootstrap":
        return _hip.particle_filter(a["kind"], a["x0"], a["theta"], a["rows"], a["values"], a["H"], a["term"], a["key"], case.dt, N,
                                    case.pos, network=a["network"], return_particles=True) + (None,)
    return _hip.guided_particle_filter(a["kind"], a["x0"], a["theta"], a["rows"], a["values"], a["H"], a["term"], a["key"], case.dt, N,
                                       case.pos, network=a["network"], return_particles=True,
                                       residual=case.proposal == "residual_bridge")


def _check_filter(case, out):
    """Scores the filter launch; returns (particles, ancestors) as float64 / int64 numpy."""
    Mf, Np, S, K, rows = case.M, case.N, case.sde.state_dim, len(case.rows), case.rows
    guided = case.proposal != "bootstrap"
    parts, anc = out[5].double().cpu().numpy(), out[6].long().cpu().numpy()
    lw_dev = out[7].double().cpu().numpy() if guided else None
    assert parts.shape == (Mf, K, Np, S) and np.isfinite(parts).all()
    assert np.array_equal(parts[:, 0], np.broadcast_to(case.x0.double().numpy()[:, None, :], (Mf, Np, S)))
    pos = list(case.pos)
    if pos:
        assert (parts[..., pos] >= fs.FLOOR).all()
        assert (parts[-1, 1:][..., pos] == fs.FLOOR).any()                    # the last filter starts at the floor: the clamp binds
    assert anc.min() >= 0 and anc.max() < Np and (np.diff(anc, axis=-1) >= 0).all()
    H = None if case.H is None else case.H.double().numpy()
    noise = forecast_noise(Mf * Np, rows[-1], S, case.key)
    theta = np.repeat(case.theta.double().numpy(), Np, axis=0)
    lws = np.empty((Mf, K, Np))
    for k in range(K):
        y = case.values[k].double().numpy()
        if k == 0 or rows[k] == rows[k - 1]:
            if k > 0:          # a shared row: the gathered particles, bit for bit
                assert np.array_equal(parts[:, k], np.take_along_axis(parts[:, k - 1], anc[:, k - 1, :, None], axis=1))
            lws[:, k] = fs.log_weights64(case, k, parts[:, k])
            if guided:         # no step since the last observation: the plain Gaussian weight
                ok = np.isfinite(lws[:, k])
                e = float(np.abs(lw_dev[:, k][ok] - lws[:, k][ok]).max())
                bound = 1e-5 * max(1.0, float(np.abs(lws[:, k][ok]).max()))
                _note(case, "filter log-weight", e / bound)
                assert e <= bound, (case.name, k, e, bound)
                lws[:, k] = lw_dev[:, k]
            continue
        start = np.take_along_axis(parts[:, k - 1], anc[:, k - 1, :, None], axis=1).reshape(Mf * Np, S)
        z = noise[:, rows[k - 1]:rows[k]]
        states, lr = fs.segment(case, start, theta, z, k)
        x64 = states[:, -1]
        e_x = float(np.abs(parts[:, k].reshape(Mf * Np, S) - x64).max() / np.abs(x64).max())
        _note(case, "filter propagation", e_x / fs.PROPAGATION_BOUND)
        print(f"{case.name} k={k} (n = {rows[k] - rows[k - 1]}): particles {e_x:.2e} of the largest magnitude")
        assert e_x < fs.PROPAGATION_BOUND, (case.name, k, e_x)
        if not guided:
            lws[:, k] = fs.log_weights64(case, k, parts[:, k])
            continue
        lw64 = fs.log_weights64(case, k, x64, lr)
        s32, lr32 = fs.segment(case, start, theta, z, k, np.float32)
        with np.errstate(all="ignore"):
            lw32 = (lr32 + fs.gauss32(y, s32[:, -1], case.variance, H)).astype(np.float64)
        ok = np.isfinite(lw64)
        got = lw_dev[:, k].reshape(Mf * Np)
        assert ok.any() and np.isfinite(got[ok]).all()
        e_k, e_32 = float(np.abs(got[ok] - lw64[ok]).max()), float(np.abs(np.where(np.isnan(lw32), -np.inf, lw32)[ok] - lw64[ok]).max())
        bound = 4.0 * e_32 + 1e-5 * max(1.0, float(np.abs(lw64[ok]).max()))
        _note(case, "filter log-weight", e_k / bound)
        print(f"{case.name} k={k}: log-weights: kernel {e_k:.2e}, fp32 reference {e_32:.2e}, bound {bound:.2e}")
        assert e_k <= bound, (case.name, k, e_k, bound)
        lws[:, k] = lw_dev[:, k]
    # weights and summaries from the kernel's particles (guided: and its own log-weights) in float64
    got = [t.double().cpu().numpy() for t in out[1:5]]
    u = ref.resampling_uniforms(Mf, K, case.key)
    e_inc = e_ess = e_mean = e_std = 0.0
    differ = n_und = 0
    for m in range(Mf):
        for k in range(K):
            lw = lws[m, k]
            inc, ess, mean, std, w = ref.observation_stage(lw, parts[m, k])
            size = (w[:, None] * np.abs(parts[m, k])).sum(axis=0) / w.sum()
            e_inc = max(e_inc, abs(got[0][m, k] - inc) / max(1.0, np.abs(lw[np.isfinite(lw)]).max()))
            e_ess = max(e_ess, abs(got[1][m, k] - ess) / ess)
            e_mean = max(e_mean, float((np.abs(got[2][m, k] - mean) / np.maximum(size, 1e-30)).max()))
            e_std = max(e_std, float((np.abs(got[3][m, k] - std) / (std + 1e-2 * size + 1e-30)).max()))
            if m < Mf - 1:
                assert ess > Np / 20, (case.name, m, k, ess)                   # there was something to compare
            d = np.abs(anc[m, k] - ref.systematic_ancestors(w, u[m, k]))
            near = fs.undecidable(w, u[m, k]) <= fs.ANCESTOR_MARGIN
            assert d.max() <= 1, (case.name, m, k, int(d.max()))
            assert not (d != 0)[~near].any(), (case.name, m, k, np.flatnonzero((d != 0) & ~near).tolist())
            differ, n_und = differ + int((d != 0).sum()), n_und + int(near.sum())
    print(f"{case.name}: increments {e_inc:.2e} (of max(1, |lw|)), ESS {e_ess:.2e}, mean {e_mean:.2e}, std {e_std:.2e} (relative); "
          f"{differ} of {anc.size} ancestors differ from float64, {n_und} undecidable")
    for q, e, b in (("increments", e_inc, 1e-5), ("ESS", e_ess, 1e-4), ("mean", e_mean, 1e-4), ("std", e_std, 1e-4)):
        _note(case, "filter " + q, e / b)
    assert e_inc < 1e-5
    assert e_ess < 1e-4 and e_mean < 1e-4 and e_std < 1e-4
    if Np == fs.N:
        _UNDECIDABLE[case.name] = (n_und, anc.size)
        assert n_und <= 2, (case.name, n_und)
    else:
        assert differ <= 1e-3 * anc.size
    assert torch.allclose(out[0].double(), out[1].double().sum(dim=1), rtol=1e-6, atol=1e-5 * float(out[1].abs().max()))
    return parts, anc


def _check_replays(case, a, out, parts, anc):
    from viforsdes_amd import _hip
    Mf, Np, S, K, rows, D = case.M, case.N, case.sde.state_dim, len(case.rows), case.rows, fs.D
    T = rows[-1]
    guided, residual = case.proposal != "bootstrap", case.proposal == "residual_bridge"
    last = fs.last_slots(case)
    tail = dict(positive_dims=case.pos, network=a["network"], n_steps=T)
    if guided:
        paths, lineage = _hip.guided_filter_replay(a["kind"], a["x0"], a["theta"], a["rows"], a["values"], a["H"], case.variance, a["key"],
                                                   case.dt, out[5], out[6], torch.from_numpy(last).to(DEV), residual=residual, **tail)
    else:
        paths, lineage = _hip.filter_replay(a["kind"], a["x0"], a["theta"], a["rows"], a["key"], case.dt, out[5], out[6],
                                            torch.from_numpy(last).to(DEV), **tail)
    paths32 = paths.cpu().numpy()
    paths, lin = paths32.astype(np.float64), lineage.long().cpu().numpy()
    assert paths.shape == (Mf, D, T + 1, S) and lin.shape == (Mf, D, K) and np.isfinite(paths).all()
    assert np.array_equal(lin[:, :, -1], last)
    for k in range(K - 1, 0, -1):                                                # the lineage: exact integer identities
        assert np.array_equal(lin[:, :, k - 1], np.take_along_axis(anc[:, k - 1], lin[:, :, k], axis=1))
    x0 = case.x0.double().numpy()
    assert np.array_equal(paths[:, :, 0], np.broadcast_to(x0[:, None, :], (Mf, D, S)))
    theta = np.repeat(case.theta.double().numpy(), D, axis=0)
    base = np.arange(Mf)[:, None] * Np
    want = np.full((Mf * D, T + 1, S), np.nan)                                   # the float64 segments, each from the kernel's store
    want[:, 0] = np.repeat(x0, D, axis=0)
    worst = worst_end = 0.0
    for k in range(K):
        t0, t1 = (rows[k - 1] if k else 0), rows[k]
        stored = np.take_along_axis(parts[:, k], lin[:, :, k, None], axis=1)
        if t1 > t0:
            start = np.repeat(x0, D, axis=0) if k == 0 else \
                np.take_along_axis(parts[:, k - 1], lin[:, :, k - 1, None], axis=1).reshape(Mf * D, S)
            z = fs.path_noise((base + lin[:, :, k]).reshape(Mf * D), case.key, T, S)[:, t0:t1]
            want[:, t0 + 1:t1 + 1] = fs.segment(case, start, theta, z, k)[0]
            seg = want[:, t0 + 1:t1 + 1]
            worst = max(worst, float(np.abs(paths[:, :, t0 + 1:t1 + 1].reshape(Mf * D, t1 - t0, S) - seg).max() / np.abs(seg).max()))
        worst_end = max(worst_end, float(np.abs(paths[:, :, t1] - stored).max() / np.abs(stored).max()))
    _note(case, "replay segments", worst / fs.PROPAGATION_BOUND)
    _note(case, "replay endpoints", worst_end / fs.PROPAGATION_BOUND)
    assert worst < fs.PROPAGATION_BOUND and worst_end < fs.PROPAGATION_BOUND, (case.name, worst, worst_end)
    if case.pos:
        assert (paths[..., list(case.pos)] >= fs.FLOOR).all()
    # the records of those draws, formed on the host from the same store: anchors, m N + slot noise paths, the filter's key
    B = Mf * D
    anchors = np.stack([np.take_along_axis(parts[:, k], lin[:, :, k, None], axis=1) for k in range(K)], axis=2).reshape(B, K, S)
    noise_path = (base[:, :, None] + lin).reshape(B, K).astype(np.uint32)
    noise_path[B - 1, K - 1] = 0xFFFFFFFF                                        # the last record is dead
    keys = np.tile(np.array(case.key, dtype=np.uint32), (B, 1))
    dv = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(DEV)
    rec = (dv(anchors.astype(np.float32)), dv(noise_path.view(np.int32)), dv(keys.view(np.int32)))
    x0_b, th_b = a["x0"].repeat_interleave(D, dim=0), a["theta"].repeat_interleave(D, dim=0)
    if guided:
        rp = _hip.guided_anchored_replay(a["kind"], x0_b, th_b, a["rows"], a["values"], a["H"], case.variance, *rec, case.dt,
                                         residual=residual, **tail)
    else:
        rp = _hip.anchored_replay(a["kind"], x0_b, th_b, a["rows"], *rec, case.dt, **tail)
    rp32 = rp.cpu().numpy()
    assert rp32.shape == (B, T + 1, S) and np.isnan(rp32[B - 1]).all() and np.isfinite(rp32[:B - 1]).all()
    e_rec = float(np.abs(rp32[:B - 1].astype(np.float64)[:, 1:] - want[:B - 1, 1:]).max() / np.abs(want[:B - 1, 1:]).max())
    same = int((rp32[:B - 1] == paths32.reshape(B, T + 1, S)[:B - 1]).all(axis=(1, 2)).sum())
    _note(case, "record replay", e_rec / fs.PROPAGATION_BOUND)
    print(f"{case.name}: replay segments {worst:.2e}, endpoints vs stored particles {worst_end:.2e}, record replay {e_rec:.2e} of the "
          f"largest magnitude; {same} of {B - 1} record paths bit-identical to the genealogy replay's")
    assert np.array_equal(rp32[:B - 1, 0], np.repeat(case.x0.numpy(), D, axis=0)[:B - 1])
    assert e_rec < fs.PROPAGATION_BOUND, (case.name, e_rec)


@pytest.mark.parametrize("case", CASES + LARGE, ids=lambda c: c.name)
def test_filter_replay_and_record_replay_match_float64_per_stage(case):
    op_elem = fs.instantiation(*case.call("filter"))
    assert op_elem[:7] == case.elem and case.N <= op_elem[7]
    a = _device_inputs(case)
    out = _filter(case, a)
    parts, anc = _check_filter(case, out)
    _check_replays(case, a, out, parts, anc)


def test_undecidable_share_and_observed_ratios():
    """The sweep's cap on the device data (asserted once every N = 64 case has run), and this run's worst error / bound per family."""
    for (family, quantity), ratio in sorted(_WORST.items()):
        print(f"{family:10s} {quantity:22s} worst error / bound {ratio:.3f}")
    if len(_UNDECIDABLE) == len(CASES):
        total, entries = (sum(v[i] for v in _UNDECIDABLE.values()) for i in (0, 1))
        print(f"{total} of {entries} resampling entries undecidable on the device data")
        assert total <= 1e-3 * entries


def test_too_many_particles_are_refused_before_any_launch():
    from viforsdes_amd import PoissonObservationLikelihood, _hip
    seen = {}
    for case in CASES:
        seen.setdefault((case.elem[0], case.elem[1], case.proposal), case)
    assert sorted(seen) == sorted(fs.refusal_classes())
    for (kind, S, proposal), case in seen.items():
        a = _device_inputs(case)
        too_many = fs.pf_max_n(kind, S, proposal != "bootstrap", proposal == "residual_bridge") + 64
        assert too_many == _hip.particle_filter_max_particles(case.kind, S, proposal=proposal) + 64
        with pytest.raises(ValueError, match="particles"):
            _filter(case, a, too_many)
        if proposal == "bootstrap":                                              # the other observation term's entry point
            counts = torch.round(case.values.abs()).to(DEV)
            other = dict(a, values=counts, term=PoissonObservationLikelihood(obs_matrix=case.H).kernel_terms(counts)
                         if case.count is None else 1.0)
            with pytest.raises(ValueError, match="particles"):
                _filter(case, other, too_many)
    torch.cuda.synchronize()
