"""Mass-action chemical reaction networks in their diffusion (chemical Langevin) approximation.

A network of S species and R reactions is given by two ``[R, S]`` tables of non-negative integers: the reactant orders
``r_ji`` (how many molecules of species i reaction j consumes) and the products (how many it makes).  Each reaction has one
rate constant, so ``theta`` is ``[.., R]``.  With the net change ``nu_j = products_j - reactants_j``:

* propensity ``h_j(x, theta) = theta_j * prod_i x_i ** r_ji`` (integer powers by repeated multiplication).  There is no
  combinatorial factor such as 1/2 for a dimerisation 2 A -> B: such constants belong in theta_j;
* drift ``f = sum_j h_j nu_j`` and covariance ``Sigma = sum_j h_j nu_j nu_j^T``;
* diffusion ``L``: the floored Cholesky factor of Sigma, column by column,
  ``L_jj = sqrt(clamp(Sigma_jj - sum_{k<j} L_jk^2, min=1e-6))`` and
  ``L_ij = (Sigma_ij - sum_{k<j} L_ik L_jk) / clamp(L_jj, min=1e-6)``.
  The floors keep singular covariances (fewer reactions than species, conservation laws) finite; at S = 2 they are the three
  clamps of ``LotkaVolterra.diffusion``.

The torch code of ``drift`` and ``diffusion`` below is the specification: it runs on any device, in any dtype and under
autograd.  Inside the kernel limits (S <= 8, R <= 16, orders <= 3) the GPU routes run the HIP kernels of
``csrc/vsde_sde_coef.h`` instead (``core.sde.builtin_sde_route``)."""
from __future__ import annotations

import operator
from collections.abc import Sequence
from typing import Optional

import torch
from torch import Tensor

MAX_ORDER = 3                 # reactant order of any species in any reaction
KERNEL_MAX_SPECIES = 8        # include/vsde_hip.h: VSDE_CRN_MAX_SPECIES
KERNEL_MAX_REACTIONS = 16     # include/vsde_hip.h: VSDE_CRN_MAX_REACTIONS
_FLOOR = 1e-6


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


def propensities(x: Tensor, sde_parameters: Tensor, reactants: Sequence[Sequence[int]]) -> Tensor:
    """``h [.., R]``: ``h_j = theta_j * prod_i x_i ** r_ji`` with the powers formed by repeated multiplication."""
    cols = []
    for j, row in enumerate(reactants):
        m = None
        for i, r in enumerate(row):
            for _ in range(r):
                m = x[..., i] if m is None else m * x[..., i]
        cols.append(sde_parameters[..., j] if m is None else sde_parameters[..., j] * m)
    return torch.stack(cols, dim=-1)


class ReactionNetworkSDE:
    """Chemical Langevin SDE of a mass-action reaction network (see the module docstring for the model).

    ``reactants`` and ``products`` are ``[R, S]`` tables of non-negative integers; ``species`` and ``reactions`` optionally
    name the S species and R reactions (used in the repr and in error messages).  ``state_dim = S``, ``sde_param_dim = R``:
    theta holds one rate constant per reaction, in the order of the rows.

    >>> sir = ReactionNetworkSDE(reactants=[[1, 1], [0, 1]], products=[[0, 2], [0, 0]], species=["S", "I"])
    >>> sir.state_dim, sir.sde_param_dim
    (2, 2)
    """

    builtin_kind = "reaction_network"  # drift / diffusion also exist as HIP kernels (csrc/vsde_sde_coef.h, kind 4)

    def __init__(self, reactants, products, species: Optional[Sequence[str]] = None,
                 reactions: Optional[Sequence[str]] = None) -> None:
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
        self.state_dim, self.sde_param_dim = S, len(r)
        self._tables: dict = {}
        self._descriptor = None

    @property
    def num_reactions(self) -> int:
        return self.sde_param_dim

    def _side(self, row) -> str:
        terms = [(f"{v} " if v > 1 else "") + self.species[i] for i, v in enumerate(row) if v > 0]
        return " + ".join(terms) if terms else "∅"

    def __repr__(self) -> str:
        rx = ", ".join(f"{name}: {self._side(a)} -> {self._side(b)}"
                       for name, a, b in zip(self.reactions, self.reactants, self.products))
        return f"ReactionNetworkSDE(species={list(self.species)}, reactions=[{rx}])"

    def _nu(self, like: Tensor) -> Tensor:
        """The net-change table ``[R, S]`` on ``like``'s device and dtype, built once per (device, dtype): an upload inside a
        captured HIP graph (the pre-training loop of a network outside the kernel limits) would break the capture."""
        key = (str(like.device), like.dtype)
        t = self._tables.get(key)
        if t is None:
            t = self._tables[key] = torch.tensor(self.change, dtype=like.dtype).to(like.device)
        return t

    def drift(self, x: Tensor, sde_parameters: Tensor) -> Tensor:
        h = propensities(x, sde_parameters, self.reactants)
        return h @ self._nu(h)

    def diffusion(self, x: Tensor, sde_parameters: Tensor) -> Tensor:
        h = propensities(x, sde_parameters, self.reactants)
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
        """Whether the HIP kernels serve this network: S <= 8, R <= 16, orders <= 3 and net changes that fit the descriptor's
        int8 entries."""
        return (self.state_dim <= KERNEL_MAX_SPECIES and self.sde_param_dim <= KERNEL_MAX_REACTIONS
                and max(max(row) for row in self.reactants) <= MAX_ORDER
                and all(-128 <= v <= 127 for row in self.change for v in row))

    def network_descriptor(self):
        """The C-ABI descriptor (``_hip.CrnNetwork``, host memory) of this network, built once."""
        if self._descriptor is None:
            from .. import _hip
            self._descriptor = _hip.crn_network(self.reactants, self.change)
        return self._descriptor
