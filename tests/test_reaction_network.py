"""ReactionNetworkSDE on the CPU: the torch specification (drift, floored Cholesky diffusion and their autograd) against
LotkaVolterra and against the covariance it factors, validation, the route to the HIP kernels (``builtin_sde_kind`` /
``builtin_sde_route``), and the reaction-network C-ABI entry points rejecting bad descriptors before any HIP call."""
import ctypes

import numpy as np
import pytest
import torch

from viforsdes_amd import ReactionNetworkSDE
from viforsdes_amd.core.euler_maruyama import euler_maruyama
from viforsdes_amd.core.sde import builtin_sde_kind, builtin_sde_route
from viforsdes_amd.examples.sdes import LotkaVolterra

LV = dict(reactants=[[1, 0], [1, 1], [0, 1]], products=[[2, 0], [0, 2], [0, 0]])
SIR = dict(reactants=[[1, 1], [0, 1]], products=[[0, 2], [0, 0]])
# 4 species: production, a dimerisation 2A -> B, a termolecular A + B + C -> D, decay, conversion, and an order-3 reaction 3C -> C + D
NET4 = dict(reactants=[[0, 0, 0, 0], [2, 0, 0, 0], [1, 1, 1, 0], [0, 0, 0, 1], [0, 1, 0, 0], [0, 0, 3, 0]],
            products=[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 1, 1]])
# S = 8 chain: 0 -> X0 -> X1 -> ... -> X7 -> 0
CHAIN8 = dict(reactants=[[0] * 8] + [[int(i == k) for i in range(8)] for k in range(8)],
              products=[[1] + [0] * 7] + [[int(i == k + 1) for i in range(8)] for k in range(8)])
ISOMER = dict(reactants=[[1, 0], [0, 1]], products=[[0, 1], [1, 0]])   # A <-> B: singular covariance


def _inputs(S, P, n=7, seed=0, lo=0.5, hi=3.0):
    g = torch.Generator().manual_seed(seed)
    x = (lo + (hi - lo) * torch.rand(n, S, generator=g, dtype=torch.float64)).requires_grad_(True)
    th = (0.2 + torch.rand(n, P, generator=g, dtype=torch.float64)).requires_grad_(True)
    return x, th


def _sigma(net, x, th):
    """Sigma = sum_j h_j nu_j nu_j^T in numpy float64, straight from the tables."""
    r, nu = np.array(net["reactants"]), np.array(net["products"]) - np.array(net["reactants"])
    x, th = x.detach().numpy(), th.detach().numpy()
    h = th * np.prod(x[:, None, :] ** r[None], axis=-1)
    return np.einsum("nr,ri,rk->nik", h, nu, nu), h @ nu


def test_network_lv_equals_lotka_volterra_f64():
    net, lv = ReactionNetworkSDE(**LV), LotkaVolterra()
    assert (net.state_dim, net.sde_param_dim) == (2, 3)
    x, th = _inputs(2, 3, n=64, seed=1, lo=0.1, hi=200.0)
    g = torch.Generator().manual_seed(2)
    gf, gG = torch.randn(64, 2, generator=g, dtype=torch.float64), torch.randn(64, 2, 2, generator=g, dtype=torch.float64)
    outs = []
    for sde in (net, lv):
        f, G = sde.drift(x, th), sde.diffusion(x, th)
        grads = torch.autograd.grad((f * gf).sum() + (G * gG).sum(), [x, th])
        outs.append((f.detach(), G.detach()) + tuple(grads))
    for a, b in zip(*outs):
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-12 * float(b.abs().max())), (a - b).abs().max()


@pytest.mark.parametrize("name", ["SIR", "NET4", "CHAIN8"])
def test_cholesky_factor_reproduces_covariance(name):
    net = {"SIR": SIR, "NET4": NET4, "CHAIN8": CHAIN8}[name]
    sde = ReactionNetworkSDE(**net)
    x, th = _inputs(sde.state_dim, sde.sde_param_dim, seed=3)
    sig, f = _sigma(net, x, th)
    L = sde.diffusion(x, th).detach().numpy()
    assert np.all(np.diagonal(L, axis1=1, axis2=2) > 1e-2)            # no floor binds
    assert np.allclose(np.triu(L, 1), 0.0)
    np.testing.assert_allclose(L @ L.transpose(0, 2, 1), sig, rtol=1e-11, atol=1e-11 * np.abs(sig).max())
    np.testing.assert_allclose(sde.drift(x, th).detach().numpy(), f, rtol=1e-12, atol=1e-12 * np.abs(f).max())


def test_singular_network_stays_finite_and_shows_the_floor():
    sde = ReactionNetworkSDE(**ISOMER)
    x, th = _inputs(2, 2, seed=4)
    L = sde.diffusion(x, th)
    f = sde.drift(x, th)
    gx, gth = torch.autograd.grad(L.sum() + f.sum(), [x, th])
    assert torch.isfinite(L).all() and torch.isfinite(gx).all() and torch.isfinite(gth).all()
    h = th[:, 0] * x[:, 0] + th[:, 1] * x[:, 1]
    assert torch.allclose(L[:, 0, 0], h.sqrt()) and torch.allclose(L[:, 1, 0], -h.sqrt())
    assert torch.all(L[:, 1, 1] == torch.tensor(1e-6, dtype=torch.float64).sqrt())   # the floor: rank-1 covariance


def test_validation_errors():
    with pytest.raises(ValueError, match="not an integer"):
        ReactionNetworkSDE(reactants=[[1.5, 0]], products=[[0, 1]])
    with pytest.raises(ValueError, match="negative"):
        ReactionNetworkSDE(reactants=[[1, 0]], products=[[0, -1]])
    with pytest.raises(ValueError, match="but products has 2"):
        ReactionNetworkSDE(reactants=[[1, 0]], products=[[0, 1], [1, 0]])
    with pytest.raises(ValueError, match="expected 2"):
        ReactionNetworkSDE(reactants=[[1, 0]], products=[[0, 1, 0]])
    with pytest.raises(ValueError, match="order 4 in species 'A'"):
        ReactionNetworkSDE(reactants=[[4, 0]], products=[[0, 1]], species=["A", "B"])
    with pytest.raises(ValueError, match="species names"):
        ReactionNetworkSDE(reactants=[[1, 0]], products=[[0, 1]], species=["A"])
    with pytest.raises(ValueError, match="at least one reaction"):
        ReactionNetworkSDE(reactants=[], products=[])
    sir = ReactionNetworkSDE(**SIR, species=["S", "I"], reactions=["infection", "removal"])
    assert "infection: S + I -> 2 I" in repr(sir) and "removal: I -> ∅" in repr(sir)


def test_builtin_kind_inside_and_outside_the_kernel_limits():
    assert builtin_sde_kind(ReactionNetworkSDE(**LV)) == "reaction_network"
    assert builtin_sde_kind(ReactionNetworkSDE(**CHAIN8)) == "reaction_network"          # S = 8, R = 9
    s9 = dict(reactants=[[int(i == k) for i in range(9)] for k in range(9)], products=[[0] * 9] * 9)
    assert builtin_sde_kind(ReactionNetworkSDE(**s9)) is None                            # S = 9
    r16 = dict(reactants=[[1, 0]] * 16, products=[[0, 1]] * 16)
    r17 = dict(reactants=[[1, 0]] * 17, products=[[0, 1]] * 17)
    assert builtin_sde_kind(ReactionNetworkSDE(**r16)) == "reaction_network"
    assert builtin_sde_kind(ReactionNetworkSDE(**r17)) is None                           # R = 17
    assert builtin_sde_kind(ReactionNetworkSDE(reactants=[[1]], products=[[200]])) is None   # change beyond int8

    class Damped(ReactionNetworkSDE):
        def drift(self, x, sde_parameters):
            return super().drift(x, sde_parameters) * 0.5

    assert builtin_sde_kind(Damped(**LV)) is None
    shadowed = ReactionNetworkSDE(**LV)
    shadowed.diffusion = lambda x, t: torch.zeros(x.shape[0], 2, 2)
    assert builtin_sde_kind(shadowed) is None

    kind, net = builtin_sde_route(ReactionNetworkSDE(**NET4))
    assert kind == "reaction_network" and (net.S, net.R) == (4, 6)
    assert net.order[2][2] == 1 and net.order[5][2] == 3 and net.change[5][3] == 1 and net.change[5][2] == -2
    assert builtin_sde_route(LotkaVolterra()) == ("lotka_volterra", None)
    assert builtin_sde_route(ReactionNetworkSDE(**r17)) == (None, None)


def test_cpu_euler_maruyama_matches_lotka_volterra():
    g = torch.Generator().manual_seed(5)
    x0 = torch.tensor([[71.0, 79.0], [40.0, 90.0], [5.0, 1.0]], dtype=torch.float64)
    th = torch.tensor([[0.5, 0.0025, 0.3], [0.6, 0.003, 0.25], [0.4, 0.002, 0.35]], dtype=torch.float64)
    noise = torch.randn(3, 200, 2, generator=g, dtype=torch.float64)
    a = euler_maruyama(ReactionNetworkSDE(**LV), x0, th, 20.0, 0.1, [0, 1], noise=noise)
    b = euler_maruyama(LotkaVolterra(), x0, th, 20.0, 0.1, [0, 1], noise=noise)
    assert torch.allclose(a, b, rtol=1e-10, atol=1e-10)


def _crn_calls(lib, net, S, P):
    """Every vsde_crn_* entry point with valid dims (S, P) and NULL data pointers: only the descriptor can fail first."""
    n, i, d = None, ctypes.c_int, ctypes.c_double
    ref = ctypes.byref(net) if net is not None else None
    return {
        "vsde_crn_sde_coefficients_fwd": (ref, i(4), i(5), i(S), i(P), n, n, n, n, n),
        "vsde_crn_sde_coefficients_bwd": (ref, i(4), i(5), i(S), i(P), n, n, n, n, n, n, n),
        "vsde_crn_euler_maruyama_fwd": (ref, i(4), i(5), i(S), i(P), n, n, n, d(0.1), n, n, n),
        "vsde_crn_euler_maruyama_bwd": (ref, i(4), i(5), i(S), i(P), n, n, n, n, d(0.1), n, n, n, n),
        "vsde_crn_forecast": (ref, i(4), i(5), i(S), i(P), i(1), n, n, n, n, d(0.1), n, n, n),
        "vsde_crn_log_weights": (ref, i(4), i(5), i(S), i(0), i(S), i(P), n, n, n, n, n, n, n, d(1.0), i(0), d(0.0), d(1.0),
                                 n, n, n, n, d(0.1), n, n),
    }


def test_abi_rejects_bad_descriptors_without_gpu():
    from viforsdes_amd import _hip
    lib = _hip.load()
    lib.vsde_last_error.restype = ctypes.c_char_p

    def good():
        return ReactionNetworkSDE(**NET4).network_descriptor()

    bad = []
    d = good(); d.S = 9; bad.append((d, 9, 6, b"9 species"))
    d = good(); d.S = 0; bad.append((d, 0, 6, b"0 species"))
    d = good(); d.R = 17; bad.append((d, 4, 17, b"17 reactions"))
    d = good(); d.R = 0; bad.append((d, 4, 0, b"0 reactions"))
    d = good(); d.order[3][1] = 4; bad.append((d, 4, 6, b"reaction 3 has order 4 in species 1"))
    d = good(); d.order[0][2] = -1; bad.append((d, 4, 6, b"order -1"))
    bad.append((good(), 3, 6, b"called with state_dim 3"))
    bad.append((good(), 4, 5, b"sde_param_dim 5"))
    bad.append((None, 4, 6, b"NULL reaction-network descriptor"))
    for net, S, P, msg in bad:
        for name, args in _crn_calls(lib, net, S, P).items():
            rc = getattr(lib, name)(*args)
            assert rc == -1, (name, msg, rc)
            assert msg in lib.vsde_last_error(), (name, msg, lib.vsde_last_error())


def test_binding_refuses_missing_descriptor():
    from viforsdes_amd import _hip
    with pytest.raises(ValueError, match="descriptor"):
        _hip._sde_entry(_hip.load(), "forecast", "reaction_network", None)
    with pytest.raises(ValueError, match="int8"):
        _hip.crn_network([[1]], [[300]])
