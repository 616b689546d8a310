"""Reaction networks shared by the kind-4 GPU tests (reactant / product tables of ReactionNetworkSDE, and for the networks with
rate laws its ``rate_laws`` / ``rate_constants``)."""
from viforsdes_amd import Hill, MichaelisMenten

LV = dict(reactants=[[1, 0], [1, 1], [0, 1]], products=[[2, 0], [0, 2], [0, 0]])
BD = dict(reactants=[[0], [1], [2]], products=[[1], [0], [1]])                     # S = 1: 0 -> X, X -> 0, 2X -> X
SIR = dict(reactants=[[1, 1], [0, 1]], products=[[0, 2], [0, 0]])
NET3 = dict(reactants=[[1, 1, 0], [0, 0, 1], [0, 0, 0], [0, 0, 0], [0, 0, 1]],    # A + B <-> C, 0 -> A, 0 -> B, C -> 0
            products=[[0, 0, 1], [1, 1, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0]])
NET4 = dict(reactants=[[0, 0, 0, 0], [2, 0, 0, 0], [1, 1, 1, 0], [0, 0, 0, 1], [0, 1, 0, 0], [0, 0, 3, 0]],
            products=[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 1, 1]])
CHAIN8 = dict(reactants=[[0] * 8] + [[int(i == k) for i in range(8)] for k in range(8)],
              products=[[1] + [0] * 7] + [[int(i == k + 1) for i in range(8)] for k in range(8)])
ISOMER = dict(reactants=[[1, 0], [0, 1]], products=[[0, 1], [1, 0]])
NETS = {"bd": BD, "sir": SIR, "net3": NET3, "net4": NET4, "chain8": CHAIN8}

# --- networks with rate laws (the KIN instantiations of the kind-4 kernels)
# S = 2: negative autoregulation (the README model): R = 4, NR = 4
AUTOREG = dict(reactants=[[0, 0], [1, 0], [1, 0], [0, 1]], products=[[1, 0], [1, 1], [0, 0], [0, 0]],
               species=["M", "P"], reactions=["transcription", "translation", "mRNA decay", "protein decay"],
               rate_laws={"transcription": Hill("P", K="K", n=2, repression=True)},
               rate_constants=["k_tx", "k_tl", 0.1, "d_P"])
# S = 3: repressilator, Hill n = 2, 3, 4 on modifiers 2, 0, 1, one shared decay rate, a fixed K: R = 6, NR = 8
REPRESS3 = dict(reactants=[[0, 0, 0]] * 3 + [[1, 0, 0], [0, 1, 0], [0, 0, 1]],
                products=[[1, 0, 0], [0, 1, 0], [0, 0, 1]] + [[0, 0, 0]] * 3,
                rate_laws={0: Hill(2, "K", n=2, repression=True), 1: Hill(0, "K", n=3, repression=True),
                           2: Hill(1, 20.0, n=4, repression=True)},
                rate_constants=["alpha", "alpha", "alpha3", "d", "d", "d"])
# S = 8: 0 -> X0 activated by X7 (n = 1, a basal feed keeps it going), X_k -> X_k+1 at v X_k / (Km + X_k), X_k -> 0: R = 16
KINETIC_CHAIN8 = dict(reactants=[[0] * 8, [0] * 8] + [[int(i == k) for i in range(8)] for k in range(7)]
                      + [[int(i == k) for i in range(8)] for k in range(7)],
                      products=[[1] + [0] * 7, [1] + [0] * 7] + [[int(i == k + 1) for i in range(8)] for k in range(7)] + [[0] * 8] * 7,
                      rate_laws={0: Hill(7, "K7", n=1), **{2 + k: MichaelisMenten(k, "Km") for k in range(7)}},
                      rate_constants=["act", 50.0] + ["v"] * 7 + ["d"] * 7)
# S = 2 with the modifier A at 0 and below: 0 -> A (keeps Sigma_AA > 0), 0 -> B activated by A, 0 -> B repressed by A, B -> 0
CLAMP2 = dict(reactants=[[0, 0], [0, 0], [0, 0], [0, 1]], products=[[1, 0], [0, 1], [0, 1], [0, 0]],
              rate_laws={1: Hill(0, "K1", n=1), 2: Hill(0, "K2", n=3, repression=True)})


# --- generated networks of the particle-filter sweep (tests/filter_sweep_reference.py): one per (species count, reaction bin of
# the kind-4 dispatch: R <= 4, R <= 8, R <= 16)
SWEEP_REACTIONS = {4: 3, 8: 7, 16: 12}


def sweep_network(S, NR, kinetic=False, R=None):
    """(ReactionNetworkSDE arguments, base theta, start state) of the sweep's network with S in 1..8 species and R = 3, 7 or 12
    reactions (NR = 4, 8, 16), or the ``R`` given (any count of the bin of NR: the SDE / jump sweep runs R = NR and the lower edges
    R = 5 and 9, tests/sde_sweep_reference.py).  Three core reactions change every species between them: the feed 0 -> X_i (i % 3 == 0), the
    first-order conversion X_0 -> X_i (i % 3 == 1; a decay at S = 1) and the second-order X_0 + X_1 -> X_i (i % 3 == 2; 2 X_0 ->
    X_0 at S = 1).  Then the decays X_i -> 0 and conversions X_i -> X_i+1, and past those the same stoichiometries again, each
    with a constant of its own.  ``kinetic``: a Hill law (repression by the last species, n = 2) on the feed, Michaelis-Menten in
    X_0 on the conversion where S > 1, one shared decay constant.  The propensities are of order 1 at the start state (a few
    molecules per unit time against populations of 6..10): with fewer reactions than species the diffusion's covariance is
    singular, and the fp32 rounding of its floored Cholesky pivots grows with the propensities."""
    R = SWEEP_REACTIONS[NR] if R is None else R
    assert {4: 1, 8: 5, 16: 9}[NR] <= R <= NR, (NR, R)
    unit = lambda *idx: [sum(int(i == j) for j in idx) for i in range(S)]
    group = lambda r: [int(i % 3 == r) for i in range(S)]
    second = unit(0, 1) if S > 1 else unit(0, 0)
    reactants = [unit(), unit(0), second]
    products = [group(0), group(1), group(2) if S > 1 else unit(0)]
    theta = [2.0, 0.1, 0.01]
    extra = [(unit(i), unit(), 0.05) for i in range(S)] + [(unit(i), unit(i + 1), 0.04) for i in range(S - 1)]
    j = 0
    while len(reactants) < R:
        a, b, k = extra[j % len(extra)]
        reactants.append(a), products.append(b), theta.append(k * (1.0 + 0.25 * (j // len(extra))))
        j += 1
    start = [6.0 + 2.0 * (i % 3) for i in range(S)]
    kw = dict(reactants=reactants, products=products)
    if kinetic:
        names = [f"k{j}" for j in range(R)]
        laws = {0: Hill(S - 1, "K", n=2, repression=True)}
        theta[0] = 4.0
        if S > 1:
            laws[1] = MichaelisMenten(0, "Km")
            theta[1] = 1.5
        for j in range(3, min(R, 3 + S)):
            names[j] = "d"                                       # the first round of decays shares one constant
        free = []
        for n, v in zip(names, theta):
            if n not in [f for f, _ in free]:
                free.append((n, v))
        free.append(("K", 8.0))
        if S > 1:
            free.append(("Km", 5.0))
        kw.update(rate_laws=laws, rate_constants=names)
        theta = [v for _, v in free]
    return kw, theta, start


# --- the cells of the SDE / jump sweep (tests/sde_sweep_reference.py) by name: sw-S<S>-NR<NR>[-k][-R<R>], "-k": with rate laws, R
# given where it is not the cell's own (R = NR at even S, SWEEP_REACTIONS[NR] at odd S)
def sweep_reactions(S, NR):
    return NR if S % 2 == 0 else SWEEP_REACTIONS[NR]


def sweep_name(S, NR, kinetic=False, R=None):
    own = R is None or R == sweep_reactions(S, NR)
    return f"sw-S{S}-NR{NR}" + ("-k" if kinetic else "") + ("" if own else f"-R{R}")


def is_sweep_name(name):
    return isinstance(name, str) and name.startswith("sw-S")


def sweep_cell(name):
    """(S, NR, kinetic, R) of a cell's name."""
    parts = name.split("-")
    S, NR = int(parts[1][1:]), int(parts[2][2:])
    R = [int(p[1:]) for p in parts[3:] if p.startswith("R")]
    return S, NR, "k" in parts[3:], R[0] if R else sweep_reactions(S, NR)
