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
