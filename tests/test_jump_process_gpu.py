"""GPU: the jump-process kernel (csrc/vsde_jump.hip) stage by stage on its own previous stage, as the filter tests do: one
flipped reaction legitimately changes everything after it, so no whole trajectory is compared.  For every logged event the state
before it is rebuilt from x0 and the kernel's own logged reactions; propensities, a0, tau and the chosen reaction are then formed
in float64 (tests/jump_process_reference.py) from the reference uniforms.

Bounds.  Waiting time: an fp32 logf, one divide and a sum of <= 16 terms give about 1e-6; 1e-5 relative is the project's fp32
scalar bound.  Reaction: equal to float64's choice unless u2 a0 lies within 1e-5 a0 of a boundary c_j (undecidable); such events
may be at most 1e-3 of all events, and the float64 reference's own share is asserted first.  Outputs, n_events and status are
bit-exact against what the kernel's own log implies.  Every call runs with max_events <= 4096."""
import numpy as np
import pytest
import torch

import jump_process_reference as ref
from jump_process_reference import check_stages, implied_by_log  # noqa: F401  (the checks the jump sweep shares)
from reaction_networks import BD, ISOMER, SIR
from viforsdes_amd import ReactionNetworkSDE, diffusion_approximation_check, jump_process

pytestmark = pytest.mark.gpu
CASES = ref.cases()
DEV = "cuda"
KEY = (123, 456)
E = 64


def run(net, xs, th, times, B, record, max_events=E):
    return jump_process(net, torch.as_tensor(xs), torch.as_tensor(th, dtype=torch.float32, device=DEV), times, n_paths=B, key=KEY,
                        max_events=max_events, record_events=record)


def same_outputs(a, b):
    return torch.equal(a.states, b.states) and torch.equal(a.n_events, b.n_events) and torch.equal(a.status, b.status)


@pytest.mark.parametrize("name", sorted(CASES))
def test_stages_per_path_inputs(name):
    """B = 300 (four full waves and a partial one), K = 4 with a zero and a duplicate time, per-path theta and x0; max_events = E,
    so that the log holds every event and the cap rule runs on the device too."""
    spec, x0, theta = CASES[name]
    net = ReactionNetworkSDE(**spec)
    assert net.kernel_compatible()
    times = [0.0, 0.25, 0.25, 1.0]
    xs, th = ref.per_path_inputs(x0, theta, 300, seed=len(name))
    th32 = th.astype(np.float32)
    res = run(net, xs, th32, times, 300, E)
    events, _ = check_stages(net, xs, th32, times, res)
    assert events > 1000
    bare = run(net, xs, th32, times, 300, 0)
    assert bare.event_times is None and bare.event_reactions is None and same_outputs(res, bare)


@pytest.mark.parametrize("B", [1, 63, 65])
@pytest.mark.parametrize("name", ["bd", "net4", "chain8", "kinetic_chain8"])
def test_stages_partial_waves_single_rows(name, B):
    """K = 1, one theta row and one x0 row for B paths: S = 1, 4, 8, R = 3, 6, 9, 16 (NR = 4, 8, 16, 16)."""
    spec, x0, theta = CASES[name]
    net = ReactionNetworkSDE(**spec)
    times = [0.5]
    res = run(net, x0, theta, times, B, E)
    xs, th32 = np.tile(np.asarray(x0, dtype=np.int64), (B, 1)), np.tile(np.asarray(theta, dtype=np.float32), (B, 1))
    check_stages(net, xs, th32, times, res)
    assert same_outputs(res, run(net, x0, theta, times, B, 0))


def test_edge_rules_on_the_device():
    f32 = dict(dtype=torch.float32, device=DEV)
    dimer = ReactionNetworkSDE(reactants=[[2]], products=[[1]])
    res = jump_process(dimer, [1], torch.tensor([3.0], **f32), [1.0, 5.0], n_paths=5, key=KEY, max_events=64)
    assert res.states.tolist() == [[[1], [1]]] * 5 and res.n_events.tolist() == [0] * 5 and res.status.tolist() == [0] * 5
    bd = ReactionNetworkSDE(**BD)
    res = jump_process(bd, [6], torch.tensor([4.0, 0.5, 0.0], **f32), [3.0], n_paths=64, key=KEY, max_events=4096, record_events=64)
    assert int(res.n_events.min()) > 0 and not bool((res.event_reactions == 2).any()) and bool(res.complete.all())
    iso = ReactionNetworkSDE(**ISOMER)
    res = jump_process(iso, [7, 3], torch.tensor([1.0, 2.0], **f32), [0.0, 0.3, 1.0, 4.0], n_paths=64, key=KEY, max_events=4096)
    assert bool((res.states.sum(dim=-1) == 10).all()) and bool((res.states >= 0).all()) and bool(res.complete.all())
    sir = ReactionNetworkSDE(**SIR)
    res = jump_process(sir, [40, 0], torch.tensor([0.01, 0.2], **f32), [0.0, 1.0, 2.0], n_paths=3, key=KEY, max_events=64,
                       record_events=4)
    assert res.states.tolist() == [[[40, 0]] * 3] * 3 and res.status.tolist() == [0] * 3 and res.n_events.tolist() == [0] * 3
    assert bool(torch.isnan(res.event_times).all()) and bool((res.event_reactions == -1).all())
    res = jump_process(bd, [5], torch.tensor([200.0, 0.1, 0.0], **f32), [0.0, 10.0, 20.0], n_paths=8, key=KEY, max_events=3,
                       record_events=8)
    assert res.status.tolist() == [1] * 8 and res.n_events.tolist() == [3] * 8 and not bool(res.complete.any())
    assert res.states[:, 0].tolist() == [[5]] * 8 and bool((res.states[:, 1:] == -1).all())
    assert bool(torch.isfinite(res.event_times[:, :3]).all()) and bool(torch.isnan(res.event_times[:, 3:]).all())
    theta = torch.tensor([[1.0, 0.5, 0.0], [1.0, -0.5, 0.0], [float("nan"), 0.5, 0.0]], **f32)
    res = jump_process(bd, [5], theta, [1.0], key=KEY, max_events=4096)
    assert res.status.tolist() == [0, 2, 2] and res.states[1:].tolist() == [[[-1]], [[-1]]]
    a = jump_process(sir, [95, 5], torch.tensor([0.02, 0.5], **f32), [1.0, 2.0], n_paths=32, key=KEY, max_events=4096)
    b = jump_process(sir, [95, 5], torch.tensor([0.02, 0.5], **f32), [1.0, 2.0], n_paths=32, key=torch.tensor(KEY), max_events=4096)
    c = jump_process(sir, [95, 5], torch.tensor([0.02, 0.5], **f32), [1.0, 2.0], n_paths=32, key=(123, 457), max_events=4096)
    assert same_outputs(a, b) and not torch.equal(a.states, c.states)
    for change in (dict(x0=[95.5, 5]), dict(x0=[-1, 5]), dict(x0=[2 ** 30 + 1, 5]), dict(times=[2.0, 1.0]), dict(times=[-1.0]),
                   dict(max_events=0), dict(max_events=2 ** 23 + 1), dict(x0=[1, 2, 3])):
        with pytest.raises(ValueError):
            jump_process(**{**dict(net=sir, x0=[95, 5], theta=torch.tensor([0.02, 0.5], **f32), times=[1.0], key=KEY), **change})


def test_exact_law_of_immigration_death_on_the_device():
    net = ReactionNetworkSDE(**BD)
    res = jump_process(net, [30], torch.tensor([10.0, 0.5, 0.0], dtype=torch.float32, device=DEV), [1.0, 2.0], n_paths=65536, key=KEY,
                       max_events=4096)
    assert bool(res.complete.all()) and int(res.n_events.max()) < 200
    for k, t in enumerate((1.0, 2.0)):
        ref.check_exact_law(res.states[:, k, 0].cpu().numpy(), 30, 10.0, 0.5, t)


def test_kernel_route_against_torch_route():
    net = ReactionNetworkSDE(**SIR)
    times, B = [0.5, 1.0, 2.0], 4096
    kernel = jump_process(net, [95, 5], torch.tensor([0.02, 0.5], dtype=torch.float32, device=DEV), times, n_paths=B, key=KEY,
                          max_events=4096)
    spec = jump_process(net, [95, 5], torch.tensor([0.02, 0.5], dtype=torch.float64, device=DEV), times, n_paths=B, key=KEY,
                        max_events=4096)
    assert bool(kernel.complete.all()) and bool(spec.complete.all()) and spec.states.is_cuda
    a, b = kernel.states.double(), spec.states.double()
    z = (a.mean(0) - b.mean(0)) / torch.sqrt(a.var(0) / B + b.var(0) / B)
    print(f"two-sample z, kernel against torch route: max |z| = {float(z.abs().max()):.3f}; "
          f"paths that differ: {int((kernel.states != spec.states).any(-1).any(-1).sum())} of {B}")
    assert float(z.abs().max()) <= 4.5


def test_network_beyond_the_kernel_limits_takes_the_torch_route():
    net = ReactionNetworkSDE(reactants=[[0] * 9] + [[int(i == k) for i in range(9)] for k in range(9)],
                             products=[[1] + [0] * 8] + [[int(i == k + 1) for i in range(9)] for k in range(9)])
    assert not net.kernel_compatible()
    res = jump_process(net, [3] * 9, torch.full((10,), 1.5, dtype=torch.float32, device=DEV), [0.2, 0.4], n_paths=16, key=KEY,
                       max_events=4096, record_events=8)
    assert res.states.is_cuda and res.states.shape == (16, 2, 9) and bool(res.complete.all()) and bool((res.states >= 0).all())
    assert int(res.n_events.min()) > 0 and bool(torch.isfinite(res.event_times[:, 0]).all())


def test_diffusion_approximation_check_on_the_device():
    net = ReactionNetworkSDE(**SIR)
    chk = diffusion_approximation_check(net, [95, 5], torch.tensor([0.004, 0.15], dtype=torch.float32, device=DEV), [5.0, 10.0], 0.05,
                                        n_paths=1024, key=KEY, max_events=4096)
    assert chk.n_incomplete == 0 and chk.jump_states.is_cuda and chk.jump_states.shape == (1024, 2, 2)
    for name in ("jump_mean", "jump_std", "diffusion_mean", "diffusion_std", "mean_shift", "std_ratio", "ks_distance", "zero_fraction"):
        assert bool(torch.isfinite(getattr(chk, name)).all()), name
    ref.check_fields(chk)
