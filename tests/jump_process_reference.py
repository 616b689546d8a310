"""numpy float64 restatement of the jump process of a reaction network (viforsdes_amd/core/jump_process.py), written
independently of the package: Gillespie's direct method, one path and one event at a time, on the uniforms of the specified
Philox stream (counter {e >> 1, 0, b, 7}; tests/philox_reference.py).

A network is taken as plain tables: ``reactants`` / ``change`` ``[R][S]`` and ``laws`` (per reaction None or ``(code, modifier
species, n)`` with code 1 = Hill activation, 2 = Hill repression); ``rates [B, 2R]`` are the effective constants
(k_0..k_{R-1}, K_0..K_{R-1}).  ``tables(net)`` reads them off a ReactionNetworkSDE."""
import math

import numpy as np

from philox_reference import _uniform, philox4x32_10


def tables(net):
    return dict(reactants=np.asarray(net.reactants, dtype=np.int64), change=np.asarray(net.change, dtype=np.int64),
                laws=[None if law is None else tuple(law[:3]) for law in net.laws])


def uniforms(paths, events, key):
    """(u1, u2) float64 arrays (broadcast of ``paths`` and ``events``): the fp32 uniforms of event e of path b, widened."""
    paths, events = np.broadcast_arrays(np.asarray(paths, dtype=np.int64), np.asarray(events, dtype=np.int64))
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    w = philox4x32_10(events >> 1, 0, paths, 7, k0, k1)
    odd = (events & 1) == 1
    return (_uniform(np.where(odd, w[2], w[0])).astype(np.float64), _uniform(np.where(odd, w[3], w[1])).astype(np.float64))


def propensities(tab, x, rates):
    """a [N, R] float64 at the integer states x [N, S] with the effective constants rates [N, 2R]."""
    x = np.asarray(x, dtype=np.int64)
    rates = np.asarray(rates, dtype=np.float64)
    R = tab["reactants"].shape[0]
    xf = x.astype(np.float64)
    a = np.empty((x.shape[0], R), dtype=np.float64)
    for j in range(R):
        row, law = tab["reactants"][j], tab["laws"][j]
        if law is None:
            m = np.ones(x.shape[0])
            for i, r in enumerate(row):
                for q in range(int(r)):
                    m = m * (xf[:, i] - q)
            a[:, j] = rates[:, j] * m
        else:
            code, s, n = law
            un, kn = xf[:, s] ** n, rates[:, R + j] ** n
            with np.errstate(invalid="ignore", divide="ignore"):
                g = (un if code == 1 else kn) / (kn + un)
            a[:, j] = rates[:, j] * g * np.all(x >= row[None, :], axis=1)
    return a


def choose(a, u2):
    """(reaction [N], undecidable [N]) for propensities a [N, R] with a0 > 0: the smallest j with u2 a0 < c_j, else the last j
    with a_j > 0; undecidable where u2 a0 is within 1e-5 a0 of some boundary c_j."""
    c = np.cumsum(a, axis=1)
    a0 = c[:, -1]
    thr = u2 * a0
    below = thr[:, None] < c
    first = below.argmax(axis=1)
    last_positive = a.shape[1] - 1 - (a[:, ::-1] > 0).argmax(axis=1)
    j = np.where(below.any(axis=1), first, last_positive)
    near = (np.abs(thr[:, None] - c) <= 1e-5 * a0[:, None]).any(axis=1)
    return j, near


def simulate(tab, x0, rates, times, key, max_events, E):
    """(states [B, K, S], n_events [B], status [B], event_times [B, E], event_reactions [B, E]) as ``jump_process`` defines them."""
    x0 = np.asarray(x0, dtype=np.int64)
    B, S = x0.shape
    times = np.asarray(times, dtype=np.float64)
    K = times.shape[0]
    states = np.full((B, K, S), -1, dtype=np.int64)
    n_events, status = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    ev_t, ev_r = np.full((B, E), np.nan), np.full((B, E), -1, dtype=np.int64)
    for b in range(B):
        x, t, k, fired = x0[b].copy(), 0.0, 0, 0
        while True:
            if fired == max_events:
                status[b] = 1
                break
            a = propensities(tab, x[None], rates[b:b + 1])[0]
            if not np.all(np.isfinite(a) & (a >= 0)) or not np.isfinite(a.sum()):
                status[b] = 2
                break
            a0 = np.cumsum(a)[-1]
            if a0 == 0:
                states[b, k:] = x
                break
            u1, u2 = uniforms(b, fired, key)
            t_next = t + -np.log(u1) / a0
            while k < K and times[k] < t_next:
                states[b, k] = x
                k += 1
            if k == K:
                break
            j = int(choose(a[None], np.asarray([u2]))[0][0])
            x = x + tab["change"][j]
            t = t_next
            if fired < E:
                ev_t[b, fired], ev_r[b, fired] = t, j
            fired += 1
        n_events[b] = fired
    return states, n_events, status, ev_t, ev_r


# --- the cases the CPU and GPU tests share: network (tests/reaction_networks.py), start state, theta in parameter_names order
def cases():
    import reaction_networks as rn
    return {
        "bd": (rn.BD, [20], [10.0, 0.5, 0.01]),
        "sir": (rn.SIR, [95, 5], [0.02, 0.5]),
        "net4": (rn.NET4, [12, 8, 6, 3], [5.0, 0.05, 0.01, 0.5, 0.3, 0.02]),                      # orders 2 and 3
        "chain8": (rn.CHAIN8, [5, 4, 3, 2, 2, 1, 1, 0], [4.0, 1.0, 0.8, 1.2, 1.0, 0.9, 1.1, 1.0, 0.7]),   # S = 8, R = 9
        "autoreg": (rn.AUTOREG, [2, 10], [5.0, 2.0, 0.3, 8.0]),                                   # Hill repression n = 2, a fixed k
        "repress3": (rn.REPRESS3, [5, 0, 10], [6.0, 4.0, 0.4, 5.0]),                              # n = 2, 3, 4, shared constants
        "kinetic_chain8": (rn.KINETIC_CHAIN8, [3, 2, 2, 1, 1, 1, 0, 0], [3.0, 4.0, 0.2, 2.0, 3.0]),   # R = 16, Hill n = 1
    }


def per_path_inputs(x0, theta, B, seed):
    """Per-path start states (x0 plus 0..2) and constants (theta times 0.8..1.2), float64, from a fixed generator."""
    rng = np.random.default_rng(seed)
    xs = np.asarray(x0, dtype=np.int64)[None, :] + rng.integers(0, 3, size=(B, len(x0)))
    th = np.asarray(theta, dtype=np.float64)[None, :] * rng.uniform(0.8, 1.2, size=(B, len(theta)))
    return xs, th


# --- the stage-by-stage checks of one kernel call with its event log (tests/test_jump_process_gpu.py, tests/test_jump_sweep_gpu.py)
KEY = (123, 456)
E = 64


def implied_by_log(tab, xs, times, ev_t, ev_r, max_events):
    """(states [B, K, S], n_events [B], status [B]) that the event log implies when it holds every event (max_events <= E):
    output k holds x0 plus the changes of the events with time <= T_k, and exists once a later event or the end was reached."""
    fired = ev_r >= 0
    n = fired.sum(axis=1)
    change = np.where(fired[:, :, None], tab["change"][np.clip(ev_r, 0, None)], 0)
    times = np.asarray(times, dtype=np.float64)
    upto = fired[:, None, :] & (ev_t[:, None, :] <= times[None, :, None])                # [B, K, E]
    states = xs[:, None, :] + np.einsum("bke,bes->bks", upto.astype(np.int64), change)
    capped = n == max_events
    last = np.where(n > 0, ev_t[np.arange(len(n)), np.clip(n - 1, 0, None)], -np.inf)
    reached = ~capped[:, None] | (times[None, :] < last[:, None])
    return np.where(reached[:, :, None], states, -1), n, capped.astype(np.int64)


def check_stages(net, xs, th32, times, res, max_events=E, key=KEY):
    """The stage-by-stage checks of one kernel call with the event log; returns (events, undecidable) for the record."""
    import torch
    tab = tables(net)
    ev_t, ev_r = res.event_times.cpu().numpy(), res.event_reactions.cpu().numpy().astype(np.int64)
    B = xs.shape[0]
    fired = ev_r >= 0
    assert np.array_equal(np.isnan(ev_t), ~fired) and ev_r.max() < tab["change"].shape[0]
    assert np.array_equal(fired, np.arange(ev_r.shape[1])[None, :] < fired.sum(axis=1)[:, None])     # a prefix of each row
    change = np.where(fired[:, :, None], tab["change"][np.clip(ev_r, 0, None)], 0)
    before = xs[:, None, :] + np.cumsum(change, axis=1) - change                                      # the state before event e
    assert (before[fired] + change[fired]).min() >= 0
    b_idx, e_idx = np.nonzero(fired)
    rates = net.kernel_parameters(torch.as_tensor(th32, dtype=torch.float32)).double().numpy()
    a = propensities(tab, before[b_idx, e_idx], rates[b_idx])
    a0 = a.sum(axis=1)
    assert a0.min() > 0
    u1, u2 = uniforms(b_idx, e_idx, key)
    # waiting time
    tau = -np.log(u1) / a0
    previous = np.where(e_idx > 0, ev_t[b_idx, np.clip(e_idx - 1, 0, None)], 0.0)
    waited = ev_t[b_idx, e_idx] - previous
    err = np.abs(waited - tau) / np.where(tau > 0, tau, 1.0)
    assert np.all(waited[tau == 0] == 0)
    # reaction
    j64, near = choose(a, u2)
    share = near.mean()
    flipped = ev_r[b_idx, e_idx] != j64
    print(f"{len(b_idx)} events: waiting-time error max {err.max():.2e}; undecidable {near.sum()} ({share:.1e}), flipped {flipped.sum()}")
    assert err.max() <= 1e-5
    assert share <= 1e-3
    assert not np.any(flipped & ~near)
    # outputs
    states, n, status = implied_by_log(tab, xs, times, ev_t, ev_r, max_events)
    assert np.array_equal(res.states.cpu().numpy(), states)
    assert np.array_equal(res.n_events.cpu().numpy(), n)
    assert np.array_equal(res.status.cpu().numpy(), status)
    assert res.states.dtype == torch.int32 and res.states.shape == (B, len(times), xs.shape[1])
    return len(b_idx), int(near.sum())


# --- the checks the CPU and GPU tests share
# exact law of immigration-death from n0: x(t) ~ Binomial(n0, e^{-death t}) + Poisson(birth / death (1 - e^{-death t}))
def immigration_death_pmf(n0, birth, death, t, size):
    p, lam = math.exp(-death * t), birth / death * (1.0 - math.exp(-death * t))
    binom = np.array([math.comb(n0, k) * p ** k * (1 - p) ** (n0 - k) for k in range(n0 + 1)])
    pois = np.exp(np.arange(size) * math.log(lam) - lam - np.array([math.lgamma(k + 1) for k in range(size)]))
    return np.convolve(binom, pois)[:size], n0 * p + lam, n0 * p * (1 - p) + lam


def check_exact_law(values, n0, birth, death, t):
    """z-score of the mean (<= 4.5) and Pearson's chi-square over the bins of expected count >= 5 (the rest pooled) against the
    Wilson-Hilferty quantile at z = 4.5; returns (z, chi-square, dof) for the record."""
    values = np.asarray(values)
    B = values.shape[0]
    pmf, mean, var = immigration_death_pmf(n0, birth, death, t, 200)
    z = (values.mean() - mean) / math.sqrt(var / B)
    expected = B * pmf
    keep = expected >= 5
    counts = np.bincount(values, minlength=200)[:200].astype(np.float64)
    obs = np.append(counts[keep], B - counts[keep].sum())
    exp = np.append(expected[keep], B - expected[keep].sum())
    chi2, dof = float(((obs - exp) ** 2 / exp).sum()), len(obs) - 1
    bound = dof * (1 - 2 / (9 * dof) + 4.5 * math.sqrt(2 / (9 * dof))) ** 3
    print(f"t = {t}: z = {z:.3f}, chi-square = {chi2:.1f} with {dof} dof (bound {bound:.1f})")
    assert abs(z) <= 4.5
    assert chi2 <= bound
    return z, chi2, dof


def ks_numpy(a, b):
    grid = np.unique(np.concatenate([a, b]))
    fa = np.searchsorted(np.sort(a), grid, side="right") / len(a)
    fb = np.searchsorted(np.sort(b), grid, side="right") / len(b)
    return np.abs(fa - fb).max()


def check_fields(chk):
    js, ds = chk.jump_states.double().cpu().numpy(), chk.diffusion_states.double().cpu().numpy()
    assert js.shape == ds.shape and js.ndim == 3
    jm, jsd, dm, dsd = js.mean(0), js.std(0), ds.mean(0), ds.std(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        shift, ratio = np.where(jsd == 0, np.nan, (dm - jm) / jsd), np.where(jsd == 0, np.nan, dsd / jsd)
    ks = np.array([[ks_numpy(js[:, k, i], ds[:, k, i]) for i in range(js.shape[2])] for k in range(js.shape[1])])
    for name, want in (("jump_mean", jm), ("jump_std", jsd), ("diffusion_mean", dm), ("diffusion_std", dsd), ("mean_shift", shift),
                       ("std_ratio", ratio), ("ks_distance", ks), ("zero_fraction", (js == 0).mean(0))):
        got = getattr(chk, name).cpu().numpy()
        assert got.shape == want.shape, name
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12, equal_nan=True, err_msg=name)
