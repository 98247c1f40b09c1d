"""The inputs and random draws of the offline evaluator's fixtures (trainlogvar_*, mvgauss_*, noisesens_*), regenerated from
their seeds — the same function as tools/make_goldens.driver_draws; the fixtures hold digests of the draws to prove it."""
import numpy as np

from oracle import recipe


def driver_draws(kind, seed, N, S, nl=4, batches=1):
    _, B, _ = recipe.inputs(seed + 60, N * batches, 3, 3, S, nl)
    rs = np.random.RandomState(seed + 61)
    out = dict(B=B)
    if kind in ("trainlogvar", "mvgauss"):
        out["dequant"] = rs.uniform(0, 1. / 127.5, (batches, N, 3, S, S)).astype(np.float32)
    if kind == "trainlogvar":
        out["eps"] = rs.normal(0, 1, (batches, N, 1, nl)).astype(np.float32)
    if kind == "mvgauss":
        _, out["B_test"], _ = recipe.inputs(seed + 62, N * batches, 3, 3, S, nl)
    if kind == "noisesens":
        out["noise"] = rs.normal(0, 1, (8, N, 3, S, S)).astype(np.float32)
    return out
