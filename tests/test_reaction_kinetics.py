"""ReactionNetworkSDE with rate laws and fixed / shared rate constants, on the CPU: the torch specification against hand-written
float64 formulas (Hill activation and repression, Michaelis-Menten), its autograd (gradcheck in x and theta, the clamp of the
modifier at 0 and below), the order of theta (``parameter_names``) and the map to the per-reaction constants
(``kernel_parameters``), a default network against today's, validation, the route to the kernels (``builtin_sde_route``), and the
six ``vsde_crn_kinetic_*`` entry points rejecting bad descriptors before any HIP call."""
import ctypes
import math

import pytest
import torch

from viforsdes_amd import Hill, MichaelisMenten, ReactionNetworkSDE
from viforsdes_amd.core import reaction_network
from viforsdes_amd.core.sde import builtin_sde_kind, builtin_sde_route, kernel_theta

# negative autoregulation: protein P represses transcription of its own mRNA M
AUTOREG = dict(reactants=[[0, 0], [1, 0], [1, 0], [0, 1]], products=[[1, 0], [1, 1], [0, 0], [0, 0]],
               species=["M", "P"], reactions=["transcription", "translation", "mRNA decay", "protein decay"],
               rate_laws={"transcription": Hill("P", K="K", n=2, repression=True)},
               rate_constants=["k_tx", "k_tl", 0.1, "d_P"])
# S -> P at V S / (K + S), and 0 -> S at a fixed rate
ENZYME = dict(reactants=[[0, 0], [1, 0]], products=[[1, 0], [0, 1]], species=["S", "P"], reactions=["feed", "conversion"],
              rate_laws={"conversion": MichaelisMenten("S", "Km")}, rate_constants=[2.0, "V"])
# two gene copies A, B with a shared decay rate; B's production activated by A (Hill n = 3, fixed K), A's repressed by B (n = 4)
TOGGLE = dict(reactants=[[0, 0], [0, 0], [1, 0], [0, 1]], products=[[1, 0], [0, 1], [0, 0], [0, 0]], species=["A", "B"],
              rate_laws={0: Hill("B", K="K_B", n=4, repression=True), 1: Hill(0, K=1.5, n=3)},
              rate_constants=["alpha", "beta", "d", "d"])
LV = dict(reactants=[[1, 0], [1, 1], [0, 1]], products=[[2, 0], [0, 2], [0, 0]])


def _x(S, n=9, seed=0, lo=0.3, hi=4.0):
    g = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(n, S, generator=g, dtype=torch.float64)


def _theta(P, n=9, seed=1):
    g = torch.Generator().manual_seed(seed)
    return 0.3 + torch.rand(n, P, generator=g, dtype=torch.float64)


# -------------------------------------------------------------------------------------------------- 1. spec vs formulas
@pytest.mark.parametrize("ratio", [0.0, 1.0, 1e4])
def test_spec_matches_hand_formulas_at_zero_half_and_saturation(ratio):
    """u = 0, u = K and u >> K for activation (n = 3, fixed K), repression (n = 4, free K) and Michaelis-Menten (free K)."""
    tog = ReactionNetworkSDE(**TOGGLE)
    assert tog.parameter_names == ("alpha", "beta", "d", "K_B")
    alpha, beta, d, KB = 1.3, 0.7, 0.2, 2.5
    th = torch.tensor([[alpha, beta, d, KB]], dtype=torch.float64)
    A, B = 1.5 * ratio, KB * ratio                         # u = ratio * K for both rate laws
    x = torch.tensor([[A, B]], dtype=torch.float64)
    h_A = alpha * KB ** 4 / (KB ** 4 + B ** 4)
    h_B = beta * A ** 3 / (1.5 ** 3 + A ** 3)
    want = torch.tensor([[h_A - d * A, h_B - d * B]], dtype=torch.float64)
    torch.testing.assert_close(tog.drift(x, th), want, rtol=1e-14, atol=1e-14)
    if ratio == 1.0:
        assert math.isclose(h_A, alpha / 2) and math.isclose(h_B, beta / 2)
    enz = ReactionNetworkSDE(**ENZYME)
    assert enz.parameter_names == ("V", "Km")
    V, Km = 3.0, 0.8
    S_ = Km * ratio
    h = V * S_ / (Km + S_)
    f = enz.drift(torch.tensor([[S_, 1.0]], dtype=torch.float64), torch.tensor([[V, Km]], dtype=torch.float64))
    torch.testing.assert_close(f, torch.tensor([[2.0 - h, h]], dtype=torch.float64), rtol=1e-14, atol=1e-14)
    G = enz.diffusion(torch.tensor([[S_, 1.0]], dtype=torch.float64), torch.tensor([[V, Km]], dtype=torch.float64))[0]
    sig = torch.tensor([[2.0 + h, -h], [-h, h]], dtype=torch.float64)      # nu = (1, 0) at 2.0, (-1, 1) at h
    if h > 1e-3:
        torch.testing.assert_close(G @ G.T, sig, rtol=1e-12, atol=1e-12)


def test_autoregulation_spec_and_the_reactant_row_adds_no_monomial():
    net = ReactionNetworkSDE(**AUTOREG)
    x, th = _x(2, seed=2), _theta(4, seed=3)
    M, P = x[:, 0], x[:, 1]
    k_tx, k_tl, d_P, K = th.unbind(-1)
    h = torch.stack([k_tx * K ** 2 / (K ** 2 + P ** 2), k_tl * M, 0.1 * M, d_P * P], -1)
    nu = torch.tensor([[1, 0], [0, 1], [-1, 0], [0, -1]], dtype=torch.float64)
    torch.testing.assert_close(net.drift(x, th), h @ nu, rtol=1e-13, atol=1e-13)
    L = net.diffusion(x, th)
    torch.testing.assert_close(L @ L.transpose(-1, -2), torch.einsum("nr,ri,rk->nik", h, nu, nu), rtol=1e-12, atol=1e-12)
    # a reactant on a rate-law reaction: S -> P at V S / (K + S) has no S^1 factor besides the law's
    enz = ReactionNetworkSDE(**ENZYME)
    xs, ts = _x(2, seed=4), _theta(2, seed=5)
    h2 = ts[:, 0] * xs[:, 0] / (ts[:, 1] + xs[:, 0])
    torch.testing.assert_close(enz.drift(xs, ts)[:, 1], h2, rtol=1e-14, atol=1e-14)


# ------------------------------------------------------------------------------------------------------------ 2. autograd
@pytest.mark.parametrize("name", ["autoreg", "enzyme", "toggle"])
def test_gradcheck_drift_and_diffusion(name):
    net = ReactionNetworkSDE(**{"autoreg": AUTOREG, "enzyme": ENZYME, "toggle": TOGGLE}[name])
    x = _x(net.state_dim, n=4, seed=6, lo=0.5, hi=3.0).requires_grad_(True)
    th = _theta(net.sde_param_dim, n=4, seed=7).requires_grad_(True)
    L = net.diffusion(x.detach(), th.detach())
    assert float(torch.diagonal(L, dim1=-2, dim2=-1).min()) > 1e-2          # no floor binds: the spec is smooth here
    assert torch.autograd.gradcheck(net.drift, (x, th))
    assert torch.autograd.gradcheck(net.diffusion, (x, th))


def test_shared_and_fixed_constants_in_the_gradient():
    tog = ReactionNetworkSDE(**TOGGLE)
    x, th = _x(2, n=5, seed=8), _theta(4, n=5, seed=9).requires_grad_(True)
    f = tog.drift(x, th)
    (g,) = torch.autograd.grad(f.sum(), th)
    torch.testing.assert_close(g[:, 2], -(x[:, 0] + x[:, 1]))               # d: shared by both decays
    kp = tog.kernel_parameters(th)
    assert kp.shape == (5, 8)
    torch.testing.assert_close(kp[:, :4], th[:, [0, 1, 2, 2]])
    torch.testing.assert_close(kp[:, 4:], torch.stack([th[:, 3], torch.full_like(th[:, 3], 1.5), torch.ones_like(th[:, 3]),
                                                       torch.ones_like(th[:, 3])], -1))
    (gk,) = torch.autograd.grad((kp * torch.arange(1.0, 9.0, dtype=torch.float64)).sum(), th)
    torch.testing.assert_close(gk, torch.tensor([[1.0, 2.0, 3.0 + 4.0, 5.0]], dtype=torch.float64).expand(5, 4))


@pytest.mark.parametrize("repression", [False, True])
@pytest.mark.parametrize("n", [1, 2])
def test_modifier_gradient_follows_the_clamp(n, repression):
    """u = clamp(x_s, min=0): at x_s = 0 the gradient passes (dg/du = n u^(n-1) c / (c+a)^2: K^-1 for n = 1, 0 for n = 2), at
    x_s < 0 it is zero and h is the value at 0."""
    net = ReactionNetworkSDE(reactants=[[0, 0]], products=[[0, 1]], rate_laws={0: Hill(0, "K", n=n, repression=repression)},
                             rate_constants=["k"])
    th = torch.tensor([[1.7, 0.6]], dtype=torch.float64)
    for xs in (0.0, -0.4):
        x = torch.tensor([[xs, 1.0]], dtype=torch.float64, requires_grad=True)
        f = net.drift(x, th)
        (g,) = torch.autograd.grad(f[0, 1], x)
        h0 = 1.7 * (1.0 if repression else 0.0)
        assert float(f[0, 1].detach()) == pytest.approx(h0, abs=1e-15)
        slope = 1.7 / 0.6 if (n == 1 and xs == 0.0) else 0.0
        assert float(g[0, 0]) == pytest.approx(-slope if repression else slope, rel=1e-14, abs=1e-15)
        assert float(g[0, 1]) == 0.0


# ----------------------------------------------------------------------------------------------- 3. theta order, defaults
def test_parameter_names_and_theta_order():
    net = ReactionNetworkSDE(**AUTOREG)
    assert net.parameter_names == ("k_tx", "k_tl", "d_P", "K") and net.sde_param_dim == 4 and not net.plain
    shared = ReactionNetworkSDE(reactants=[[1, 0], [0, 1], [0, 0]], products=[[0, 0], [0, 0], [0, 1]],
                                rate_laws={2: Hill(0, K="K1", n=1), 1: Hill(1, K="d")}, rate_constants=["d", "d", "v"])
    assert shared.parameter_names == ("d", "v", "K1")                     # "d" also serves as reaction 1's K
    th = torch.tensor([[0.5, 2.0, 3.0]], dtype=torch.float64)
    torch.testing.assert_close(shared.kernel_parameters(th), torch.tensor([[0.5, 0.5, 2.0, 1.0, 0.5, 3.0]], dtype=torch.float64))
    named = ReactionNetworkSDE(reactants=[[1]], products=[[0]], reactions=["decay"])
    assert named.parameter_names == ("decay",) and named.plain
    fixed_only = ReactionNetworkSDE(reactants=[[1]], products=[[0]], rate_constants=[0.25])
    assert fixed_only.parameter_names == () and fixed_only.sde_param_dim == 0
    f = fixed_only.drift(torch.tensor([[2.0]], dtype=torch.float64), torch.zeros(1, 0, dtype=torch.float64))
    assert float(f) == -0.5
    assert "parameters=['k_tx', 'k_tl', 'd_P', 'K']" in repr(net)


def test_default_network_is_todays():
    new = ReactionNetworkSDE(**LV)
    assert new.plain and new.sde_param_dim == 3 and new.num_reactions == 3 and new.parameter_names == ("R0", "R1", "R2")
    x, th = _x(2, seed=10, lo=1.0, hi=50.0), _theta(3, seed=11) * 0.01
    h = reaction_network.propensities(x, th, new.reactants)
    nu = torch.tensor(new.change, dtype=torch.float64)
    assert torch.equal(new.drift(x, th), h @ nu)
    # the same model through the rate-law machinery: identical numbers, one more route
    mapped = ReactionNetworkSDE(**LV, rate_constants=["a", "b", "c"], rate_laws={})
    assert mapped.plain and builtin_sde_route(mapped)[1] is mapped.network_descriptor()
    assert torch.equal(mapped.drift(x, th), new.drift(x, th)) and torch.equal(mapped.diffusion(x, th), new.diffusion(x, th))
    renamed = ReactionNetworkSDE(**LV, rate_constants=["b", "a", "c"])      # theta follows first appearance: still plain
    assert renamed.plain and renamed.parameter_names == ("b", "a", "c")
    shared = ReactionNetworkSDE(**LV, rate_constants=["a", "b", "a"])
    assert not shared.plain and shared.parameter_names == ("a", "b")
    ths = th[:, :2]
    torch.testing.assert_close(shared.drift(x, ths), new.drift(x, ths[:, [0, 1, 0]]), rtol=0, atol=0)
    torch.testing.assert_close(shared.diffusion(x, ths), new.diffusion(x, ths[:, [0, 1, 0]]), rtol=0, atol=0)


# ---------------------------------------------------------------------------------------------------------- 4. validation
def test_validation_messages():
    base = dict(reactants=[[0, 0], [1, 0]], products=[[1, 0], [0, 0]], species=["A", "B"], reactions=["make", "lose"])
    cases = [
        (dict(rate_laws={"grow": Hill("A", "K")}), "unknown reaction 'grow'"),
        (dict(rate_laws={2: Hill("A", "K")}), "reaction index 2 does not exist"),
        (dict(rate_laws={"make": Hill("C", "K")}), "unknown species 'C'"),
        (dict(rate_laws={"make": Hill(2, "K")}), "unknown species 2"),
        (dict(rate_laws={"make": Hill("B", "K", n=5)}), "Hill coefficient n = 5 must be an integer in 1..4"),
        (dict(rate_laws={"make": Hill("B", "K", n=0)}), "Hill coefficient n = 0"),
        (dict(rate_laws={"make": Hill("B", "K", n=1.5)}), "Hill coefficient n = 1.5"),
        (dict(rate_laws={"make": Hill("B", 0.0)}), "fixed K = 0.0 must be > 0"),
        (dict(rate_laws={"make": Hill("B", -1.0)}), "fixed K = -1.0 must be > 0"),
        (dict(rate_laws={"make": Hill("B", float("inf"))}), "must be finite"),
        (dict(rate_laws={"make": ("B", "K")}), "expected Hill"),
        (dict(rate_laws={"make": Hill("B", "K"), 0: Hill("B", "K")}), "two rate laws"),
        (dict(rate_constants=["a"]), "rate_constants has 1 entries for 2 reactions"),
        (dict(rate_constants=["a", -0.5]), "reaction 'lose': fixed value -0.5 must be >= 0"),
        (dict(rate_constants=["a", float("nan")]), "must be finite"),
        (dict(rate_constants=["a", None]), "neither a parameter name nor a number"),
    ]
    for kw, msg in cases:
        with pytest.raises(ValueError, match=msg.replace("(", r"\(").replace(".", r"\.")):
            ReactionNetworkSDE(**base, **kw)


# ------------------------------------------------------------------------------------------------------------- 5. routing
def test_routing_keeps_the_two_tuple_contract():
    from viforsdes_amd import _hip
    kind, net = builtin_sde_route(ReactionNetworkSDE(**LV))
    assert kind == "reaction_network" and isinstance(net, _hip.CrnNetwork)
    ar = ReactionNetworkSDE(**AUTOREG)
    route = builtin_sde_route(ar)
    assert len(route) == 2 and route[0] == "reaction_network"
    r = route[1]
    assert isinstance(r, _hip.CrnKineticRoute) and r is builtin_sde_route(ar)[1]          # built once
    assert (r.network.S, r.network.R) == (2, 4)
    assert list(r.kinetics.law)[:4] == [2, 0, 0, 0] and r.kinetics.modifier[0] == 1 and r.kinetics.hill_n[0] == 2
    th = _theta(4, n=3).float()
    torch.testing.assert_close(kernel_theta(r, th), ar.kernel_parameters(th))
    assert kernel_theta(net, th) is th and kernel_theta(None, th) is th
    # the limits
    assert builtin_sde_kind(ReactionNetworkSDE(**TOGGLE)) == "reaction_network"
    r17 = dict(reactants=[[1, 0]] * 17, products=[[0, 1]] * 17)
    assert builtin_sde_route(ReactionNetworkSDE(**r17, rate_constants=["k"] * 17)) == (None, None)    # P = 1, R = 17
    r16 = dict(reactants=[[1, 0]] * 16, products=[[0, 1]] * 16)
    big = ReactionNetworkSDE(**r16, rate_laws={j: Hill(1, f"K{j}", n=4) for j in range(16)})
    assert big.sde_param_dim == 32 and builtin_sde_kind(big) == "reaction_network"
    s9 = dict(reactants=[[int(i == k) for i in range(9)] for k in range(9)], products=[[0] * 9] * 9)
    assert builtin_sde_kind(ReactionNetworkSDE(**s9, rate_laws={0: Hill(8, "K")})) is None


# ------------------------------------------------------------------------------------------------------------------ 6. ABI
def _kinetic_calls(lib, net, kin, S, P):
    """Every vsde_crn_kinetic_* entry point with valid dims and NULL data pointers: only the descriptors can fail first."""
    n, i, d = None, ctypes.c_int, ctypes.c_double
    a = (ctypes.byref(net) if net is not None else None, ctypes.byref(kin) if kin is not None else None)
    return {
        "vsde_crn_kinetic_sde_coefficients_fwd": a + (i(4), i(5), i(S), i(P), n, n, n, n, n),
        "vsde_crn_kinetic_sde_coefficients_bwd": a + (i(4), i(5), i(S), i(P), n, n, n, n, n, n, n),
        "vsde_crn_kinetic_euler_maruyama_fwd": a + (i(4), i(5), i(S), i(P), n, n, n, d(0.1), n, n, n),
        "vsde_crn_kinetic_euler_maruyama_bwd": a + (i(4), i(5), i(S), i(P), n, n, n, n, d(0.1), n, n, n, n),
        "vsde_crn_kinetic_forecast": a + (i(4), i(5), i(S), i(P), i(1), n, n, n, n, d(0.1), n, n, n),
        "vsde_crn_kinetic_log_weights": a + (i(4), i(5), i(S), i(0), i(S), i(4), i(P), n, n, n, n, n, n, n, n, d(1.0), i(0),
                                             d(0.0), d(1.0), n, n, n, n, d(0.1), n, n),
    }


def test_abi_rejects_bad_kinetic_descriptors_without_gpu():
    from viforsdes_amd import _hip
    lib = _hip.load()
    lib.vsde_last_error.restype = ctypes.c_char_p
    ar = ReactionNetworkSDE(**AUTOREG)                  # S = 2, R = 4: P = 2R = 8

    def good():
        r = ar.kernel_descriptor()
        net, kin = _hip.CrnNetwork(), _hip.CrnKinetics()
        ctypes.memmove(ctypes.byref(net), ctypes.byref(r.network), ctypes.sizeof(net))
        ctypes.memmove(ctypes.byref(kin), ctypes.byref(r.kinetics), ctypes.sizeof(kin))
        return net, kin

    bad = []
    net, kin = good(); kin.law[0] = 3; bad.append((net, kin, 2, 8, b"reaction 0 has law code 3"))
    net, kin = good(); kin.law[2] = -1; bad.append((net, kin, 2, 8, b"reaction 2 has law code -1"))
    net, kin = good(); kin.modifier[0] = 2; bad.append((net, kin, 2, 8, b"reaction 0 has modifier species 2 (0..1 for 2 species)"))
    net, kin = good(); kin.modifier[0] = -1; bad.append((net, kin, 2, 8, b"modifier species -1"))
    net, kin = good(); kin.hill_n[0] = 5; bad.append((net, kin, 2, 8, b"reaction 0 has Hill coefficient 5 (1..4 supported)"))
    net, kin = good(); kin.hill_n[0] = 0; bad.append((net, kin, 2, 8, b"Hill coefficient 0"))
    net, kin = good(); bad.append((net, kin, 2, 4, b"called with state_dim 2 and 4 effective constants (2R = 8)"))
    net, kin = good(); bad.append((net, kin, 2, 9, b"9 effective constants"))
    net, kin = good(); bad.append((net, kin, 3, 8, b"called with state_dim 3"))
    net, kin = good(); net.S = 9; bad.append((net, kin, 9, 8, b"9 species"))
    net, kin = good(); bad.append((net, None, 2, 8, b"NULL rate-law descriptor"))
    bad.append((None, good()[1], 2, 8, b"NULL reaction-network descriptor"))
    for net, kin, S, P, msg in bad:
        for name, args in _kinetic_calls(lib, net, kin, S, P).items():
            rc = getattr(lib, name)(*args)
            assert rc == -1, (name, msg, rc)
            assert msg in lib.vsde_last_error(), (name, msg, lib.vsde_last_error())
    # mass-action rows ignore modifier / n; rows >= R are ignored
    net, kin = good()
    kin.modifier[1], kin.hill_n[1], kin.law[7] = 7, 0, 9
    for name, args in _kinetic_calls(lib, net, kin, 2, 8).items():
        rc = getattr(lib, name)(*args)
        assert rc == -1 and b"NULL argument" in lib.vsde_last_error(), (name, lib.vsde_last_error())


def test_binding_descriptor_checks():
    from viforsdes_amd import _hip
    with pytest.raises(ValueError, match="rate-law descriptor"):
        _hip.crn_kinetics([(1, 0, 5)])
    with pytest.raises(ValueError, match="rate-law descriptor"):
        _hip.crn_kinetics([(4, 0, 1)])
    lib = _hip.load()
    fn, net, kin = _hip._sde_entry(lib, "forecast", "reaction_network", ReactionNetworkSDE(**AUTOREG).kernel_descriptor())
    assert fn.__name__ == "vsde_crn_kinetic_forecast"
