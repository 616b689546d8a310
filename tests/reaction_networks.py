"""Reaction networks shared by the kind-4 GPU tests (reactant / product tables of ReactionNetworkSDE)."""
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
