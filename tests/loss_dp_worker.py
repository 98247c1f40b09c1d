"""Worker of the optional losses' forced-exchange tests: two AugmentedCycleGAN steps with a loss on, alone or
(ACGAN_DIST_FORCE=1, one rank) with every collective of the data-parallel exchange run anyway.
usage: loss_dp_worker.py <out.npz> <train_instance|supervised_train_instance> <options as JSON>"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dtgan_amd  # noqa: E402,F401
from dtgan_amd import dist as D, model as M, ops  # noqa: E402
from hip_util import load_recipe, t  # noqa: E402
from model_cases import make_opt  # noqa: E402
from oracle import recipe  # noqa: E402

out, step, options = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
assert step in ("train_instance", "supervised_train_instance"), step
if D._FORCE:
    D.init_from_env(os.environ.get("ACGAN_DP_BACKEND", "nccl"))
ops.set_precision("f32")
opt = make_opt(input_nc=3, output_nc=3, ngf=8, nef=8, ndf=8, nlatent=4, n_blocks=2, **options)
torch.manual_seed(1)
m = M.AugmentedCycleGAN(opt, testing=True)
for k, net in m._net_dict().items():
    load_recipe(net, k, 7, "rich")
A, B, z = recipe.inputs(9, 4, 3, 3, 64, 4)
res = {}
for st in range(2):
    if step == "supervised_train_instance":
        vals = m.supervised_train_instance(t(A), t(B), t(z))
        res["s%d/names" % st] = np.array(list(vals.keys()))
        res["s%d/values" % st] = np.array(list(vals.values()))
    else:
        losses, visuals, gnorms = m.train_instance(t(A), t(B), t(z))
        res["s%d/names" % st] = np.array(list(losses.keys()))
        res["s%d/losses" % st] = np.array(list(losses.values()))
        res["s%d/gnorms" % st] = np.array(list(gnorms.values()))
res["forced"] = np.array(int(D.exchange_on()))
np.savez(out, **res)
print("done")
