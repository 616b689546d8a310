"""The kind-4 sweep of the SDE-side and jump kernels: a pure-Python mirror of ``crn_dispatch``
(csrc/vsde_sde_coef.h), the 48 instantiations ``<4, S, NR, KIN>`` every kernel behind it is compiled at (S 1..8, NR 4 / 8 / 16,
mass action and rate laws), and one generated network per instantiation.  Nothing here needs a GPU.

Cases.  The network of a cell is ``reaction_networks.sweep_network(S, NR, kinetic, R)``: at even S it has R = NR reactions (the
``j < R`` guard of the unrolled loops is always true and ``crn_store_rates`` writes all NR registers), at odd S R = 3, 7, 12.  Two
more points sit on the lower edge of a bin, (S 6, R 5) and (S 7, R 9), each in both forms: 52 cases.  A case is named
``sw-S<S>-NR<NR>[-k][-R<R>]``, and ``sde_reference.crn_sde`` / ``EM_KINDS`` and ``sde_aux_reference.KINDS`` take that name, so
the case builders, references and magnitudes of those two modules serve the sweep as they serve the named networks.

Inputs: the network's own constants and start state (populations 6..10, propensities of order 1), each jittered by +-20 %, noise
0.01 N(0, 1), dt = 0.05.  The floored pivots of a cell are read off the float64 reference (``sde_reference.sweep_floored``):

    cells                                      floored pivots     zeroed
    NR 4, S 5 (R 3) and S 6 (R 4)              2                  noise / g_diffusion columns of the floored pivots
    NR 4, S 7 (R 3) and S 8 (R 4)              4                  the same
    NR 8, S 6, R 5 (the lower-edge point)      1                  nothing: the path through a floored column is scored
    every other cell                           0                  nothing

Each row in both forms.  With two or more floored pivots the adjoint divides the forward's rounding noise by the floored
c = 1e-3 twice, and no float64 comparison can score that; with one it is divided once and stays within the bound.

Clamp sites as in ``sde_reference.em_case``.  The clamped species is the last one (full rank) or species 2 (cells with floored
pivots, ``sde_reference.sweep_hit_dim``), kicked by -EM_BIG k with the smallest integer k that makes the kick at least 22 at the
start state; it leaves the floor on its drift alone (every species of these networks has an inflow), not on a kick back: the
last pivot of a network with about as many reactions as species cancels a few hundred times, and an unclamped kick through it
put the float32 adjoint at 30 to 60 times the magnitude's rounding.

The forecast starts the clamped species of every other path at U(0, 1e-3).  The log weights take a trajectory of the network
itself (``sde_aux_reference.lw_case``: float64 Euler-Maruyama under 0.5 N(0, 1) increments, the floored columns zeroed as above,
z = softplus^-1(x)), so that no residual has a component of order 1 along a floored direction, and their quadratic form to first
order; tests/test_sde_sweep_bounds.py asserts per case that an all-zero output misses C_LW.

Magnitudes: those of sde_reference / sde_aux_reference, with the diffusion factor's taken as the smaller of the recursion's and
the first-order perturbation of a Cholesky factor (``sde_reference._first_order_factor``: the recursion's alone reaches 1e120
times the entry in the last rows of these networks, and a bound made from it holds a kernel to nothing).

Bounds: the constants of sde_reference / sde_aux_reference, and two of this module's own for the families that miss an existing
one, 4 x their worst CPU ratio (tests/test_sde_sweep_bounds.py asserts that float32 torch stays within c / 4 on every case and
that the two still reject injected defects; the MI355X column is what tests/test_sde_sweep_gpu.py printed, never used to set c):

    launch                          constant                    worst CPU ratio    worst ratio on an MI355X
    em_fwd, S != 2                  C_EM_STEP        10.5        2.57               4.48
    em_fwd, S  = 2                  C_EM_STEP_S2     15.5        3.77               3.01
    em_bwd                          C_EM_ADJ_CRN     120        18.48               3.90
    coef_fwd, mass action           C_COEF_FWD       13.5        3.07               3.07
    coef_fwd, rate laws             C_COEF_FWD_KIN   16          3.98               3.98
    coef_bwd                        C_COEF_VJP_CRN   83         12.44              12.95
    forecast                        C_FC_STEP_CRN    18          3.31               3.23
    log_weight                      C_LW             28          0.37               0.33

The S = 2 cells have a constant of their own for the step: their clamped species is X_1, the one product species that is also a
reactant of the second-order reaction, and the step from the floor, 1e-6 + f dt, has nothing but the cancelling drift sum of up
to 16 reactions in its magnitude.  The rate-law cells have one for the coefficients: a Hill / Michaelis-Menten propensity makes
three or four roundings more than the mass-action product its magnitude stands for.

The jump kernels run the same networks (second half of this module; tests/test_jump_sweep.py, tests/test_jump_sweep_gpu.py), and
so does the jump-segment replay kernel (last part; DESIGN section 3.33, tests/test_jump_replay_sweep.py,
tests/test_jump_replay_sweep_gpu.py).
"""
import functools

import numpy as np

import reaction_networks as rn
import sde_aux_reference as A
import sde_reference as R

CRN_MAX_S, CRN_MAX_R = 8, 16
BINS = (4, 8, 16)
C_EM_STEP_S2 = 15.5          # 4 x 3.77, rounded up (module docstring)
C_COEF_FWD_KIN = 16.0        # 4 x 3.98


def dispatch(S, R_, kinetic):
    """``(NS, NR, KIN)``: the template arguments ``route_dispatch`` / ``crn_dispatch`` pick for a network of S species and R_
    reactions, with rate laws or without -- or a string, the reason ``crn_net`` refuses it."""
    if not 1 <= S <= CRN_MAX_S:
        return f"reaction network: {S} species"
    if not 1 <= R_ <= CRN_MAX_R:
        return f"reaction network: {R_} reactions"
    return (S, 4 if R_ <= 4 else 8 if R_ <= 8 else CRN_MAX_R, bool(kinetic))


CELLS = [(S, NR, kin) for kin in (False, True) for NR in BINS for S in range(1, CRN_MAX_S + 1)]
EDGE_POINTS = ((6, 5), (7, 9))          # (S, R) on the lower edge of a bin, in both forms


def cases():
    """(S, R, kinetic) of every case: one per cell, then the lower-edge points."""
    out = [(S, rn.sweep_reactions(S, NR), kin) for S, NR, kin in CELLS]
    return out + [(S, R_, kin) for S, R_ in EDGE_POINTS for kin in (False, True)]


def name_of(S, R_, kinetic):
    return rn.sweep_name(S, dispatch(S, R_, kinetic)[1], kinetic, R_)


NAMES = [name_of(*c) for c in cases()]


def em_shape(name):
    """(B, T) of the simulator launches: a full 64-path group and a group of one path; two chunk seams and a partial chunk."""
    return 65, 2 * R.EM_KINDS[name][2] + 3


COEF_SHAPE = (1, 257)
FC_SHAPE = (65, 9, "all")
FC_SUBSETS = ((1, 4, 5), (9, 9))
LW_B, LW_T, LW_K = 2, 257, 5


def em_step_c(name):
    return C_EM_STEP_S2 if rn.sweep_cell(name)[0] == 2 else R.C_EM_STEP


def coef_fwd_c(name):
    return C_COEF_FWD_KIN if rn.sweep_cell(name)[2] else A.C_COEF_FWD


def lw_shape(name):
    """The log-weight case of a cell: every state dim positive, the five rows of ``lw_rows``, the observation matrix and the theta
    mask varied with the species count."""
    S = rn.sweep_cell(name)[0]
    return (name, S, LW_B, LW_T, "all", LW_K, A.LW_OBS[S % 3], A.LW_TMASKS[S % 3], S % 2, None)


def floored_counts():
    """{name: number of floored pivots} over the cases."""
    return {n: len(R.sweep_floored(n)) for n in NAMES}


# ============================================================================================================ jump kernels
# The same cases on the exact jump process (csrc/vsde_jump.hip: jump_kernel<S, NR, KIN>, csrc/vsde_jump_filter.hip: jf_kernel): the
# integer start state of sweep_network, per-path constants and start states of jump_process_reference.per_path_inputs.
JUMP_B, JUMP_E = 65, 64
JUMP_TIMES = [0.0, 0.25, 0.25, 1.0]
JF_M, JF_N, JF_BIG_N = 3, 64, 1024
JF_MAX_EVENTS = 4096
JF_RATE_SCALE = 2.0
JF_LIKES = ("gaussian", "poisson", "nb")
JF_BIG = [rn.sweep_name(S, 16, kin) for S in (1, 8) for kin in (False, True)]      # S 1 and 8, both forms, NR 16, again at N = 1024
ANCESTOR_MARGIN = 1e-5          # tests/filter_sweep_reference.py

# per case, in the order of NAMES, the key salt ``find_salts`` found: the first for which the float64 run alone meets the
# conditions of tests/test_jump_sweep.py (jump: at least 200 events, no path at the cap, undecidable reactions at most 1e-3 of
# the events; filter: ESS > N / 20 at every observation, no resampling threshold within ANCESTOR_MARGIN of a cumulative sum,
# flagged (particle, segment) pairs at most 2e-2).  No kernel output enters.
JUMP_SALTS = (1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0,
              0, 0, 0, 0, 0, 0, 0, 0)
JF_SALTS = (1, 2, 0, 0, 2, 0, 0, 0, 1, 0, 1, 1, 0, 3, 1, 0, 0, 2, 1, 0, 0, 0, 2, 0, 0, 0, 0, 0, 3, 0, 1, 0, 1, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0,
            1, 0, 0, 0, 1, 0, 3, 1)
JF_BIG_SALTS = (0, 0, 0, 0)


def _salt(table, i):
    return table[i] if i < len(table) else 0


@functools.lru_cache(maxsize=None)
def jump_net(name):
    from viforsdes_amd import ReactionNetworkSDE
    S, NR, kinetic, R_ = rn.sweep_cell(name)
    kw, theta, start = rn.sweep_network(S, NR, kinetic, R_)
    return ReactionNetworkSDE(**kw), theta, [int(v) for v in start]


def jump_case(name, salt=None):
    """(net, xs int64 [B, S], th32 [B, P], times, key) of the jump_kernel call of a case."""
    import jump_process_reference as jref
    i = NAMES.index(name)
    net, theta, start = jump_net(name)
    xs, th = jref.per_path_inputs(start, theta, JUMP_B, seed=100 + i)
    salt = _salt(JUMP_SALTS, i) if salt is None else salt
    return net, xs, th.astype(np.float32), JUMP_TIMES, (123 + 1000 * salt, 456 + i)


def jump_conditions(name, salt=None):
    """The float64 run of a jump case alone: events fired, whether a path reached the cap, the undecidable reaction choices."""
    import torch
    import jump_process_reference as jref
    net, xs, th32, times, key = jump_case(name, salt)
    tab = jref.tables(net)
    rates = net.kernel_parameters(torch.as_tensor(th32)).double().numpy()
    states, n, status, ev_t, ev_r = jref.simulate(tab, xs, rates, times, key, JUMP_E, JUMP_E)
    fired = ev_r >= 0
    change = np.where(fired[:, :, None], tab["change"][np.clip(ev_r, 0, None)], 0)
    before = xs[:, None, :] + np.cumsum(change, axis=1) - change
    b_idx, e_idx = np.nonzero(fired)
    a = jref.propensities(tab, before[b_idx, e_idx], rates[b_idx])
    near = jref.choose(a, jref.uniforms(b_idx, e_idx, key)[1])[1]
    events = int(n.sum())
    return dict(events=events, capped=int((status != 0).sum()), undecidable=int(near.sum()),
                ok=events >= 200 and not (status != 0).any() and near.sum() <= 1e-3 * events)


def filter_case(name, big=False, salt=None):
    """(net, theta fp32 [M, P] (torch), xs [M, S], ys [K, O], likelihood spec of jump_filter_reference, key, N) of the jf_kernel call
    of a case: Gaussian, Poisson and negative-binomial terms alternate over the cases; the observations sit near the start state."""
    import torch
    import jump_process_reference as jref
    i = NAMES.index(name)
    net, theta, start = jump_net(name)
    # the rate constants doubled (the half-saturation constants kept): the four times span one unit of time in two segments of
    # positive length, and the kernel check asks for more events than (particle, segment) pairs
    fast = [v if n in ("K", "Km") else JF_RATE_SCALE * v for n, v in zip(net.parameter_names, theta)]
    xs, th = jref.per_path_inputs(start, fast, JF_M, seed=200 + i)
    kind = JF_LIKES[i % 3]
    like = {"gaussian": ("gaussian", 25.0, None), "poisson": ("poisson", 0.9, None), "nb": ("nb", 5.0, 1.0, None)}[kind]
    rng = np.random.default_rng(300 + i)
    ys = np.round(np.asarray(start, dtype=np.float64)[None, :] + rng.integers(0, 3, size=(len(JUMP_TIMES), len(start))))
    salt = (_salt(JF_BIG_SALTS, JF_BIG.index(name)) if big else _salt(JF_SALTS, i)) if salt is None else salt
    key = ((0x9E3779B9 ^ (i * 2654435761)) & 0xFFFFFFFF, (0x7F4A7C15 + 7919 * salt + (1 << 20) * int(big)) & 0xFFFFFFFF)
    return net, torch.from_numpy(th).float(), xs, ys, like, key, JF_BIG_N if big else JF_N


def filter_conditions(name, big=False, salt=None):
    """The float64 filter of a case alone (tests/jump_filter_reference.py): smallest ESS, stopped particles, resampling entries
    within ANCESTOR_MARGIN of a cumulative sum, flagged (particle, segment) pairs."""
    import filter_sweep_reference as fs
    import jump_filter_reference as jf
    import jump_process_reference as jref
    import particle_filter_reference as pref
    net, th, xs, ys, like, key, N = filter_case(name, big, salt)
    rates = net.kernel_parameters(th.double()).numpy()
    out = jf.run_filter(jref.tables(net), xs, rates, JUMP_TIMES, ys, like, N, key, JF_MAX_EVENTS, vectorized=True)
    u = pref.resampling_uniforms(JF_M, len(JUMP_TIMES), key)
    ess, und = float(out["ess"].min()), 0
    for m in range(JF_M):
        for k in range(len(JUMP_TIMES)):
            lw = out["log_weights"][m, k]
            und += int((fs.undecidable(np.exp(lw - lw.max()), u[m, k]) <= ANCESTOR_MARGIN).sum())
    flagged, pairs = int(out["undecidable"].sum()), out["undecidable"].size
    stopped = int(out["stopped"].sum())
    # N = 1024: a threshold lies within 1e-5 of one of 1024 cumulative sums for 2 % of the entries whatever the key, so the large
    # cells keep the kernel check's own cap (at most 1e-3 of the ancestors differ from float64), as the large cells of the
    # particle-filter sweep do
    ok = ess > N / 20 and stopped == 0 and flagged <= 2e-2 * pairs and (big or und == 0)
    return dict(ess=ess, stopped=stopped, undecidable=und, flagged=flagged, pairs=pairs, events=int(out["events"].sum()), ok=ok)


def find_salts(conditions, names, tries=200, **kw):
    """Per case the first key salt whose float64 run meets ``conditions`` (-1: none in ``tries``)."""
    return tuple(next((s for s in range(tries) if conditions(n, salt=s, **kw)["ok"]), -1) for n in names)


# ====================================================================================================== jump-segment replay
# The same cases on the replay kernel (csrc/vsde_jump_replay.hip: jr_kernel<S, NR, KIN, ANCHORED>; DESIGN section 3.33;
# tests/test_jump_replay_sweep.py, tests/test_jump_replay_sweep_gpu.py): the filter case of a cell, D = 22 draws per filter whose final
# slots come from a seeded generator, the output times of tests/jump_smoother_reference.py.
JR_D = 22                       # B K = 3 * 22 * 4 = 264 threads: a full 256-thread block and a block of 8; B = 66 is no power of two
JR_CAP = 4096                   # = JF_MAX_EVENTS: no segment stops
JR_SMALL_CAP = 4                # the smallest cap at which the float64 replay alone meets ``replay_conditions`` and the two sweep-wide
#                                 conditions of tests/test_jump_replay_sweep.py (``find_small_cap`` reproduces it)
JR_INTERIOR = ((1, 0, 3), (2, 0, 3), (4, 3, 6), (5, 3, 6))      # (interior output, the observation-time outputs on either side)


def last_slots(name):
    """last_slot int32 [M, D] of a case: every row holds slot 0, slot N - 1, one slot twice and one -1 (a dead draw among live
    ones), at positions shuffled per row."""
    rng = np.random.default_rng(400 + NAMES.index(name))
    rows = rng.integers(0, JF_N, size=(JF_M, JR_D))
    rows[:, 0], rows[:, 1], rows[:, 3], rows[:, 4] = 0, JF_N - 1, rows[:, 2], -1
    return np.stack([row[rng.permutation(JR_D)] for row in rows]).astype(np.int32)


def replay_case(name, salt=None):
    """``filter_case(name)`` and the final slots: (net, theta fp32 [M, P] (torch), xs [M, S], ys, likelihood, key, N, last_slot)."""
    return filter_case(name, salt=salt) + (last_slots(name),)


@functools.lru_cache(maxsize=None)
def replay_lineages(name, salt=None):
    """The float64 filter of a case alone and the records along the lineages of ``last_slots``: (tab, times, path times, the
    arguments (x0, rates, anchors, noise_path, keys) of ``jump_smoother_reference.replay_records``).  No kernel output enters."""
    import jump_filter_reference as jf
    import jump_process_reference as jref
    import jump_smoother_reference as js
    net, th, xs, ys, like, key, N, last = replay_case(name, salt)
    tab = jref.tables(net)
    rates = net.kernel_parameters(th.double()).numpy()
    flt = jf.run_filter(tab, xs, rates, JUMP_TIMES, ys, like, N, key, JF_MAX_EVENTS, vectorized=True)
    assert int(flt["stopped"].sum()) == 0
    lineage = js.trace(flt["ancestors"], last)
    return tab, JUMP_TIMES, js.REPLAY_PATH_TIMES, js.records_of_lineage(flt["particles"], lineage, xs, rates, key)


@functools.lru_cache(maxsize=None)
def replay_reference(name, cap, salt=None):
    import jump_smoother_reference as js
    tab, times, path_times, records = replay_lineages(name, salt)
    return js.replay_records(tab, *records, times, path_times, cap)


def replay_conditions(name, cap, salt=None):
    """What the float64 replay of a case shows at the event cap ``cap``: flagged pairs, segments by status, whether some interior
    output differs from the outputs at both neighbouring observation times in some record, and the status-1 segments that wrote
    some of their outputs / none of them (among those that own any)."""
    import jump_smoother_reference as js
    out = replay_reference(name, cap, salt)
    p, st = out["paths"], out["status"]
    begin = js.ownership(js.REPLAY_PATH_TIMES, JUMP_TIMES)
    live = replay_lineages(name, salt)[3][3][:, -1] != js.DEAD_PATH
    moved = any(bool(((p[live, q] != p[live, a]).any(axis=1) & (p[live, q] != p[live, b]).any(axis=1) & (p[live, q] >= 0).all(axis=1)).any())
                for q, a, b in JR_INTERIOR)
    partial = empty = 0
    for k in range(st.shape[1]):
        own = p[:, begin[k]:begin[k + 1]]
        if own.shape[1]:
            written = (own >= 0).all(axis=2).sum(axis=1)
            partial += int(((st[:, k] == 1) & (written > 0) & (written < own.shape[1])).sum())
            empty += int(((st[:, k] == 1) & (written == 0)).sum())
    by_status = np.bincount(st[live].reshape(-1), minlength=3).tolist()
    flagged, pairs = int(out["undecidable"].sum()), st.size
    # a complete segment of three events: with the cap's stopped segments it has drawn both halves of the first Philox block and
    # from the second (``e >> 1`` = 0, 0, 1, 1)
    three = bool(((st == 0) & (out["n_events"] == 3)).any())
    ok = flagged <= js.CAP * pairs and (by_status[1:] == [0, 0] and moved if cap == JR_CAP else by_status[0] > 0 and by_status[1] > 0)
    return dict(flagged=flagged, pairs=pairs, by_status=by_status, moved=moved, partial=partial, empty=empty, three=three,
                events=int(out["n_events"].sum()), ok=ok)


def find_small_cap(tries=8, second_block=True):
    """The smallest cap in 1 .. tries at which every case meets ``replay_conditions`` and the sweep shows a status-1 segment that
    wrote some of its outputs and one that wrote none (-1: no such cap).  ``second_block``: every case also shows a complete
    segment of three events, so that complete and stopped segments both reach the second Philox block; without it a cap of 1
    would do, at which no segment ever takes the odd half of a block."""
    for cap in range(1, tries + 1):
        cs = [replay_conditions(n, cap) for n in NAMES]
        if all(c["ok"] and (c["three"] or not second_block) for c in cs) and sum(c["partial"] for c in cs) > 0 and sum(c["empty"] for c in cs) > 0:
            return cap
    return -1
