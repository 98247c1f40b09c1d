"""Worker for tests/test_hip_fss_loss_step.py: two paired AugmentedCycleGAN steps with the fss term on, alone or
(ACGAN_DIST_FORCE=1, one rank) with every collective of the data-parallel exchange run anyway.
usage: fss_loss_dp_worker.py <out.npz>"""
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
from oracle import recipe  # noqa: E402
from test_hip_step import make_opt  # noqa: E402

if D._FORCE:
    D.init_from_env(os.environ.get("ACGAN_DP_BACKEND", "nccl"))
ops.set_precision("f32")
thr = [[0.0, 0.5]] * 3
opt = make_opt(input_nc=3, output_nc=3, ngf=8, nef=8, ndf=8, nlatent=4, n_blocks=2, lambda_fss_A=0.2, lambda_fss_B=0.1,
               fss_loss_windows=(3, 9), fss_tau=0.05, fss_loss_thr_A=thr, fss_loss_thr_B=thr)
torch.manual_seed(1)
m = M.AugmentedCycleGAN(opt, testing=True)
for k, net in m._net_dict().items():
    load_recipe(net, k, 7, "rich")
A, B, z = recipe.inputs(9, 4, 3, 3, 64, 4)
res = {}
for st in range(2):
    vals = m.supervised_train_instance(t(A), t(B), t(z))
    res["s%d/names" % st] = np.array(list(vals.keys()))
    res["s%d/values" % st] = np.array(list(vals.values()))
res["forced"] = np.array(int(D.exchange_on()))
np.savez(sys.argv[1], **res)
print("done")
