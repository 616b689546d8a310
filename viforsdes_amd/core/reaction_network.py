"""Chemical reaction networks in their diffusion (chemical Langevin) approximation.

A network of S species and R reactions is given by two ``[R, S]`` tables of non-negative integers: the reactant orders
``r_ji`` (how many molecules of species i reaction j consumes) and the products (how many it makes).  By default each reaction
has one free rate constant, so ``theta`` is ``[.., R]``; ``rate_constants`` may instead fix a constant or share one parameter
between reactions, and ``rate_laws`` may give a reaction a Hill or Michaelis-Menten rate law, whose half-saturation constant K
is a parameter too (``parameter_names`` is then the order of theta).  With the net change ``nu_j = products_j - reactants_j``
and the rate constant ``k_j``:

* propensity of a mass-action reaction ``h_j = k_j * prod_i x_i ** r_ji`` (integer powers by repeated multiplication).  There
  is no combinatorial factor such as 1/2 for a dimerisation 2 A -> B: such constants belong in k_j;
* propensity of a reaction with a rate law on the modifier species s, ``u = clamp(x_s, min=0)``: ``h_j = k_j * g`` with
  ``g = u^n / (K^n + u^n)`` (activation) or ``K^n / (K^n + u^n)`` (repression), n in 1..4; the reactant row of such a reaction
  sets its net change and adds no monomial (``S -> P`` at ``V S / (K + S)``);
* drift ``f = sum_j h_j nu_j`` and covariance ``Sigma = sum_j h_j nu_j nu_j^T``;
* diffusion ``L``: the floored Cholesky factor of Sigma, column by column,
  ``L_jj = sqrt(clamp(Sigma_jj - sum_{k<j} L_jk^2, min=1e-6))`` and
  ``L_ij = (Sigma_ij - sum_{k<j} L_ik L_jk) / clamp(L_jj, min=1e-6)``.
  The floors keep singular covariances (fewer reactions than species, conservation laws) finite; at S = 2 they are the three
  clamps of ``LotkaVolterra.diffusion``.

The torch code of ``drift`` and ``diffusion`` below is the specification: it runs on any device, in any dtype and under
autograd.  Inside the kernel limits (S <= 8, R <= 16, orders <= 3, Hill coefficients <= 4) the GPU routes run the HIP kernels
of ``csrc/vsde_sde_coef.h`` instead (``core.sde.builtin_sde_route``); the kernels take the per-reaction constants
(``kernel_parameters``), the map from theta stays in torch."""
from __future__ import annotations

import math
import operator
from collections.abc import Mapping, Sequence
from dataclasses import dataclass
from typing import Optional, Union

import torch
from torch import Tensor

MAX_ORDER = 3                 # reactant order of any species in any reaction
KERNEL_MAX_SPECIES = 8        # include/vsde_hip.h: VSDE_CRN_MAX_SPECIES
KERNEL_MAX_REACTIONS = 16     # include/vsde_hip.h: VSDE_CRN_MAX_REACTIONS
MAX_HILL = 4                  # include/vsde_hip.h: VSDE_CRN_MAX_HILL
LAW_HILL_ACTIVATION, LAW_HILL_REPRESSION = 1, 2   # include/vsde_hip.h: VSDE_CRN_LAW_* (0: mass action)
_FLOOR = 1e-6


@dataclass(frozen=True)
class Hill:
    """Hill rate law of one reaction: ``h = k * u^n / (K^n + u^n)`` (activation) or ``k * K^n / (K^n + u^n)`` (repression),
    ``u = clamp(x[species], min=0)``.  ``species`` is the modifier (a species name or index); ``K`` names a free parameter
    (sharable like the rate constants) or is a fixed float > 0; ``n`` is an integer in 1..4."""
    species: Union[str, int]
    K: Union[str, float]
    n: int = 1
    repression: bool = False


def MichaelisMenten(species: Union[str, int], K: Union[str, float]) -> Hill:
    """Michaelis-Menten kinetics ``h = V * u / (K + u)``: ``Hill(species, K, n=1)``, V being the reaction's rate constant."""
    return Hill(species, K, n=1)


def _int_table(name: str, rows) -> tuple[tuple[int, ...], ...]:
    rows = rows.tolist() if hasattr(rows, "tolist") else rows
    try:
        table = tuple(tuple(row) for row in rows)
    except TypeError:
        raise ValueError(f"{name} must be a [reactions, species] table of integers") from None
    out = []
    for j, row in enumerate(table):
        vals = []
        for i, v in enumerate(row):
            if isinstance(v, bool):
                raise ValueError(f"{name}[{j}][{i}] = {v!r} is not an integer")
            try:
                iv = operator.index(v)
            except TypeError:
                raise ValueError(f"{name}[{j}][{i}] = {v!r} is not an integer") from None
            if iv < 0:
                raise ValueError(f"{name}[{j}][{i}] = {iv} is negative")
            vals.append(iv)
        out.append(tuple(vals))
    return tuple(out)


def propensities(x: Tensor, sde_parameters: Tensor, reactants: Sequence[Sequence[int]], laws=None) -> Tensor:
    """``h [.., R]``: ``h_j = theta_j * prod_i x_i ** r_ji`` with the powers formed by repeated multiplication.

    With ``laws`` (per reaction None, or ``(law code, modifier species, n)`` of a Hill law), ``sde_parameters`` are the
    effective constants ``[.., 2R]`` (``ReactionNetworkSDE.kernel_parameters``: k_0..k_{R-1}, K_0..K_{R-1}) and a rate-law
    reaction's propensity is ``k_j * a / (c + a)`` (activation) or ``k_j * c / (c + a)`` (repression) with ``a = u^n``,
    ``c = K_j^n`` by repeated multiplication, ``u = clamp(x_s, min=0)``: the kernels' operation order."""
    R = len(reactants)
    cols = []
    for j, row in enumerate(reactants):
        law = laws[j] if laws is not None else None
        if law is not None:
            code, s, n = law
            u = x[..., s].clamp(min=0)
            K = sde_parameters[..., R + j]
            a, c = u, K
            for _ in range(n - 1):
                a, c = a * u, c * K
            cols.append(sde_parameters[..., j] * ((a if code == LAW_HILL_ACTIVATION else c) / (c + a)))
            continue
        m = None
        for i, r in enumerate(row):
            for _ in range(r):
                m = x[..., i] if m is None else m * x[..., i]
        cols.append(sde_parameters[..., j] if m is None else sde_parameters[..., j] * m)
    return torch.stack(cols, dim=-1)


class ReactionNetworkSDE:
    """Chemical Langevin SDE of a reaction network (see the module docstring for the model).

    ``reactants`` and ``products`` are ``[R, S]`` tables of non-negative integers; ``species`` and ``reactions`` optionally
    name the S species and R reactions (used in the repr, in error messages and as keys of ``rate_laws``).

    ``rate_constants`` (optional, one entry per reaction): a ``str`` names a free parameter (the same name twice is one shared
    parameter), a finite float >= 0 is a fixed constant that never appears in theta.  The default gives one free constant per
    reaction, named after the reaction.  ``rate_laws`` (optional) maps a reaction (name or index) to a ``Hill`` /
    ``MichaelisMenten`` law; reactions without one are mass action.  theta holds the free names in order of first appearance,
    over ``rate_constants`` in reaction order and then over the rate laws' K in reaction order: ``parameter_names``,
    ``sde_param_dim = len(parameter_names)``.  ``state_dim = S``.

    >>> sir = ReactionNetworkSDE(reactants=[[1, 1], [0, 1]], products=[[0, 2], [0, 0]], species=["S", "I"])
    >>> sir.state_dim, sir.sde_param_dim
    (2, 2)
    >>> ar = ReactionNetworkSDE(reactants=[[0, 0], [1, 0], [1, 0], [0, 1]], products=[[1, 0], [1, 1], [0, 0], [0, 0]],
    ...                         species=["M", "P"], reactions=["transcription", "translation", "mRNA decay", "protein decay"],
    ...                         rate_laws={"transcription": Hill("P", K="K", n=2, repression=True)},
    ...                         rate_constants=["k_tx", "k_tl", 0.1, "d_P"])
    >>> ar.parameter_names
    ('k_tx', 'k_tl', 'd_P', 'K')
    """

    builtin_kind = "reaction_network"  # drift / diffusion also exist as HIP kernels (csrc/vsde_sde_coef.h, kind 4)

    def __init__(self, reactants, products, species: Optional[Sequence[str]] = None,
                 reactions: Optional[Sequence[str]] = None, rate_laws: Optional[Mapping] = None,
                 rate_constants: Optional[Sequence[Union[str, float]]] = None) -> None:
        r, p = _int_table("reactants", reactants), _int_table("products", products)
        if len(r) == 0:
            raise ValueError("a reaction network needs at least one reaction")
        if len(p) != len(r):
            raise ValueError(f"reactants has {len(r)} reactions but products has {len(p)}")
        S = len(r[0])
        if S == 0:
            raise ValueError("a reaction network needs at least one species")
        for name, table in (("reactants", r), ("products", p)):
            for j, row in enumerate(table):
                if len(row) != S:
                    raise ValueError(f"{name}[{j}] has {len(row)} entries, expected {S} (one per species)")
        self.species = tuple(species) if species is not None else tuple(f"x{i}" for i in range(S))
        self.reactions = tuple(reactions) if reactions is not None else tuple(f"R{j}" for j in range(len(r)))
        if len(self.species) != S:
            raise ValueError(f"{len(self.species)} species names for {S} species")
        if len(self.reactions) != len(r):
            raise ValueError(f"{len(self.reactions)} reaction names for {len(r)} reactions")
        for j, row in enumerate(r):
            for i, v in enumerate(row):
                if v > MAX_ORDER:
                    raise ValueError(f"reaction {self.reactions[j]!r} has order {v} in species {self.species[i]!r}; "
                                     f"mass-action orders above {MAX_ORDER} are not supported")
        self.reactants, self.products = r, p
        self.change = tuple(tuple(pj - rj for pj, rj in zip(prow, rrow)) for prow, rrow in zip(p, r))
        self.laws = self._resolve_laws(rate_laws)
        self.parameter_names, self._sources = self._resolve_parameters(rate_constants)
        self.state_dim, self.sde_param_dim = S, len(self.parameter_names)
        # mass action with one free constant per reaction in reaction order: theta is the rate constants themselves
        self.plain = (all(law is None for law in self.laws) and len(self.parameter_names) == len(r)
                      and all(src == ("theta", j) for j, src in enumerate(self._sources[:len(r)])))
        self._tables: dict = {}
        self._maps: dict = {}
        self._descriptor = None
        self._route = None

    @property
    def num_reactions(self) -> int:
        return len(self.reactants)

    def _reaction_index(self, key) -> int:
        if isinstance(key, str):
            if key not in self.reactions:
                raise ValueError(f"rate_laws: unknown reaction {key!r} (reactions: {list(self.reactions)})")
            return self.reactions.index(key)
        if isinstance(key, bool):
            raise ValueError(f"rate_laws: {key!r} is not a reaction name or index")
        try:
            j = operator.index(key)
        except TypeError:
            raise ValueError(f"rate_laws: {key!r} is not a reaction name or index") from None
        if not 0 <= j < len(self.reactants):
            raise ValueError(f"rate_laws: reaction index {j} does not exist ({len(self.reactants)} reactions)")
        return j

    def _resolve_laws(self, rate_laws) -> tuple:
        """Per reaction None (mass action) or ``(law code, modifier species, n, K)`` with K a name or a fixed float."""
        laws: list = [None] * len(self.reactants)
        for key, law in (rate_laws or {}).items():
            j = self._reaction_index(key)
            name = self.reactions[j]
            if laws[j] is not None:
                raise ValueError(f"rate_laws: reaction {name!r} is given two rate laws")
            if not isinstance(law, Hill):
                raise ValueError(f"rate law of reaction {name!r}: expected Hill(...) or MichaelisMenten(...), got {law!r}")
            sp = law.species
            if isinstance(sp, str):
                if sp not in self.species:
                    raise ValueError(f"rate law of reaction {name!r}: unknown species {sp!r} (species: {list(self.species)})")
                s = self.species.index(sp)
            else:
                try:
                    s = operator.index(sp) if not isinstance(sp, bool) else -1
                except TypeError:
                    s = -1
                if not 0 <= s < len(self.species):
                    raise ValueError(f"rate law of reaction {name!r}: unknown species {sp!r} "
                                     f"(a name or an index in 0..{len(self.species) - 1})")
            n = law.n
            if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= MAX_HILL:
                raise ValueError(f"rate law of reaction {name!r}: Hill coefficient n = {n!r} must be an integer in 1..{MAX_HILL}")
            K = law.K
            if not isinstance(K, str):
                Kf = _fixed_value(K, f"rate law of reaction {name!r}: K")
                if not Kf > 0:
                    raise ValueError(f"rate law of reaction {name!r}: fixed K = {K!r} must be > 0")
                K = Kf
            elif not K:
                raise ValueError(f"rate law of reaction {name!r}: K must be a non-empty parameter name or a float > 0")
            laws[j] = (LAW_HILL_REPRESSION if law.repression else LAW_HILL_ACTIVATION, s, n, K)
        return tuple(laws)

    def _resolve_parameters(self, rate_constants) -> tuple:
        """(parameter names in theta order, 2R sources): ``("theta", p)`` or ``("fixed", value)`` for k_0..k_{R-1}, K_0..K_{R-1}."""
        R = len(self.reactants)
        names: list = []
        sources: list = []
        if rate_constants is None:          # theta_j = k_j, named after the reaction (names need not be distinct)
            names, sources = list(self.reactions), [("theta", j) for j in range(R)]
            rate_constants = ()
        else:
            rate_constants = list(rate_constants)
            if len(rate_constants) != R:
                raise ValueError(f"rate_constants has {len(rate_constants)} entries for {R} reactions")

        def source(spec, what):
            if isinstance(spec, str):
                if not spec:
                    raise ValueError(f"{what}: a parameter name must not be empty")
                if spec not in names:
                    names.append(spec)
                return ("theta", names.index(spec))
            return ("fixed", _fixed_value(spec, what))

        for j, spec in enumerate(rate_constants):
            src = source(spec, f"rate constant of reaction {self.reactions[j]!r}")
            if src[0] == "fixed" and not src[1] >= 0:
                raise ValueError(f"rate constant of reaction {self.reactions[j]!r}: fixed value {spec!r} must be >= 0")
            sources.append(src)
        for j, law in enumerate(self.laws):
            sources.append(("fixed", 1.0) if law is None else source(law[3], f"rate law of reaction {self.reactions[j]!r}: K"))
        return tuple(names), tuple(sources)

    def _side(self, row) -> str:
        terms = [(f"{v} " if v > 1 else "") + self.species[i] for i, v in enumerate(row) if v > 0]
        return " + ".join(terms) if terms else "∅"

    def __repr__(self) -> str:
        rx = ", ".join(f"{name}: {self._side(a)} -> {self._side(b)}"
                       for name, a, b in zip(self.reactions, self.reactants, self.products))
        if self.plain:
            return f"ReactionNetworkSDE(species={list(self.species)}, reactions=[{rx}])"
        return f"ReactionNetworkSDE(species={list(self.species)}, reactions=[{rx}], parameters={list(self.parameter_names)})"

    def _nu(self, like: Tensor) -> Tensor:
        """The net-change table ``[R, S]`` on ``like``'s device and dtype, built once per (device, dtype): an upload inside a
        captured HIP graph (the pre-training loop of a network outside the kernel limits) would break the capture."""
        key = (str(like.device), like.dtype)
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = torch.tensor(self.change, dtype=like.dtype).to(like.device)
        return t

    def kernel_parameters(self, theta: Tensor) -> Tensor:
        """The per-reaction effective constants ``[.., 2R]`` of theta ``[.., P]``: the rate constants k_0..k_{R-1}, then the
        half-saturation constants K_0..K_{R-1} (1 for mass-action reactions), fixed values included.  One index gather from
        tensors cached per (device, dtype), so it is differentiable (autograd sums the gradients of shared parameters) and
        capturable in a HIP graph."""
        key = (str(theta.device), theta.dtype)
        m = self._maps.get(key)
        if m is None:
            P = len(self.parameter_names)
            fixed = [v for kind, v in self._sources if kind == "fixed"]
            idx, f = [], 0
            for kind, v in self._sources:
                if kind == "theta":
                    idx.append(v)
                else:
                    idx.append(P + f)
                    f += 1
            m = self._maps[key] = (torch.tensor(idx, dtype=torch.long).to(theta.device),
                                   torch.tensor(fixed, dtype=theta.dtype).to(theta.device))
        idx, fixed = m
        ext = torch.cat([theta, fixed.expand(*theta.shape[:-1], fixed.shape[0])], dim=-1)
        return ext.index_select(-1, idx)

    def _propensities(self, x: Tensor, sde_parameters: Tensor) -> Tensor:
        if self.plain:
            return propensities(x, sde_parameters, self.reactants)
        return propensities(x, self.kernel_parameters(sde_parameters), self.reactants,
                            tuple(None if law is None else law[:3] for law in self.laws))

    def drift(self, x: Tensor, sde_parameters: Tensor) -> Tensor:
        h = self._propensities(x, sde_parameters)
        return h @ self._nu(h)

    def diffusion(self, x: Tensor, sde_parameters: Tensor) -> Tensor:
        h = self._propensities(x, sde_parameters)
        nu = self._nu(h)
        sigma = torch.einsum("...r,ri,rk->...ik", h, nu, nu)
        S = self.state_dim
        L = [[None] * S for _ in range(S)]
        for j in range(S):
            s = sigma[..., j, j]
            for k in range(j):
                s = s - L[j][k] * L[j][k]
            L[j][j] = torch.sqrt(s.clamp(min=_FLOOR))
            c = L[j][j].clamp(min=_FLOOR)
            for i in range(j + 1, S):
                a = sigma[..., i, j]
                for k in range(j):
                    a = a - L[i][k] * L[j][k]
                L[i][j] = a / c
        zero = torch.zeros_like(L[0][0])
        return torch.stack([torch.stack([L[i][k] if k <= i else zero for k in range(S)], dim=-1) for i in range(S)], dim=-2)

    def kernel_compatible(self) -> bool:
        """Whether the HIP kernels serve this network: S <= 8, R <= 16, orders <= 3, net changes that fit the descriptor's
        int8 entries, and rate laws with a modifier among the S species and a Hill coefficient in 1..4."""
        return (self.state_dim <= KERNEL_MAX_SPECIES and self.num_reactions <= KERNEL_MAX_REACTIONS
                and max(max(row) for row in self.reactants) <= MAX_ORDER
                and all(-128 <= v <= 127 for row in self.change for v in row)
                and all(law is None or (0 <= law[1] < self.state_dim and 1 <= law[2] <= MAX_HILL) for law in self.laws))

    def network_descriptor(self):
        """The C-ABI descriptor (``_hip.CrnNetwork``, host memory) of this network, built once."""
        if self._descriptor is None:
            from .. import _hip
            self._descriptor = _hip.crn_network(self.reactants, self.change)
        return self._descriptor

    def kernel_descriptor(self):
        """What the kernel routes take (built once): the ``_hip.CrnNetwork`` of a plain network (mass action, theta = the rate
        constants), else a ``_hip.CrnKineticRoute`` carrying the network and rate-law descriptors and ``kernel_parameters``."""
        if self.plain:
            return self.network_descriptor()
        if self._route is None:
            from .. import _hip
            kin = _hip.crn_kinetics([None if law is None else law[:3] for law in self.laws])
            self._route = _hip.CrnKineticRoute(self.network_descriptor(), kin, self.kernel_parameters)
        return self._route


def _fixed_value(v, what: str) -> float:
    if isinstance(v, bool):
        raise ValueError(f"{what} = {v!r} is neither a parameter name nor a number")
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what} = {v!r} is neither a parameter name nor a number") from None
    if not math.isfinite(f):
        raise ValueError(f"{what}: fixed value {v!r} must be finite")
    return f
