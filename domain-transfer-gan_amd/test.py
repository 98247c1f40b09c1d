import argparse
import math
import os
import pickle
import random
import time

import numpy as np
import torch

from . import ops
from .dataloader import AlignedIterator, UnalignedIterator, centre_windows, load_numpy_data
from .eval_metrics import METRICS, WHOLE_FIELD_METRICS, _eval_splits
from .evaluate import eval_mse_A, eval_ubo_B, one_to_three_channels
from .model import AugmentedCycleGAN, StochCycleGAN, gauss_reparametrize, kld_std_guss
from .modules import _starts_with_conv
from .options import REFERENCE_METRICS, TestOptions, check_overlap
from .train import save_image_grid

# The module's documentation, put together here: the project's own metrics (eval_metrics.METRICS) each carry their paragraph
# beside their code, and the metric names are written once.
__doc__ = """Offline evaluation of a trained checkpoint — Py3 counterpart of /root/reference/augmented_cyclegan/test.py.

    python -m dtgan_amd.test --chk_path <expr_dir>/latest --dataroot <npz dir> --metric """ + "|".join(REFERENCE_METRICS + tuple(m.name for m in METRICS)) + """

The saved options of the run are read from opt.pkl next to the checkpoint (or opt.txt, parse_opt_file), the model is rebuilt
with testing=True, seeded with 12345 and loaded.  Metrics (test.py:230-283):
  bpp         the variational bound on B (evaluate.eval_ubo_B, --ubo_steps iterates per test batch of 200), after training the
              per-pixel log-variance logvar_B on the first 20 % of the training data (--train_logvar 1, train_logvar)
  mse         B -> A mean squared error on dev and test
  visual      cycle / multi / cycle-B-multi / multi-cycle (/ inference) grids of every dev batch of 10
  noise_sens  |B - rec_B| per sample after perturbing fake_A with eight noise levels -> <res_dir>/noise_sens.npy
  mvgauss     the multivariate-Gaussian baseline bpp (compute_bpp_MVGauss_B, test.py:123-134; new as a --metric)
""" + "\n".join(m.doc for m in METRICS) + """

A run trained with --native_res (its saved options say so) is scored by every other metric on what it was trained on: the
centre grid_size windows of the stored fields in place of resized ones.

--ema 1 loads the averaged weights of a run trained with --ema_decay (the checkpoint's ema_<net> entries) into the networks
instead of the live ones; every metric then runs unchanged.  A checkpoint without them ends the run with a message.

Deviations from the reference:
  * the pixel count is C*H*W of the data, not the hard-coded 64*64*3;
  * every output file goes under res_dir (the reference writes noise_sens.npy to the working directory);
  * no stray exit() after the first cycle grid (test.py:294) — every grid of every dev batch is written;
  * data is the project's .npz layout through dataloader.load_numpy_data (the reference imports a missing
    edges2shoes_data module, test.py:8); batch sizes are capped at the size of the split;
  * parse_opt_file splits an opt.txt line at its first ':' only;
  * the likelihood sums and gradients of the bound, train_logvar and the MVGauss baseline run on the HIP kernels
    (ops.PixelNLL).
"""

NOISE_STDS = (0, 0.1, 0.2, 0.5, 1, 2, 3, 5)      # test.py:101


def parse_val(s):
    """test.py:301-317"""
    if s == 'None':
        return None
    if s == 'True':
        return True
    if s == 'False':
        return False
    if s == 'inf':
        return float('inf')
    try:
        f = float(s)
        if '.' in s:
            return f
        i = int(f)
        return i if i == f else f
    except ValueError:
        return s


def parse_opt_file(opt_path):
    """test.py:299-330: the options dict of a training run from its opt.pkl or opt.txt"""
    if opt_path.endswith('pkl'):
        with open(opt_path, 'rb') as f:
            return dict(pickle.load(f))
    opt = dict()
    with open(opt_path) as f:
        for line in f:
            if line.startswith('-----') or not line.strip():
                continue
            k, v = line.split(':', 1)
            opt[k.strip()] = parse_val(v.strip())
    return opt


def _grid(images, path, nrow):
    """(n, C, H, W) images in [-1, 1], any C <= 3 -> PNG grid (test.py's vutils.save_image(normalize=True, range=(-1, 1)))"""
    save_image_grid(one_to_three_channels(images.detach().float().cpu())[:, :3], path, nrow)


def visualize_cycle(opt, real_A, visuals, name):
    """test.py:16-22"""
    size = real_A.size()
    images = [one_to_three_channels(img.cpu()).unsqueeze(1) for img in visuals.values()]
    _grid(torch.cat(images, dim=1).view(size[0] * len(images), 3, size[2], size[3]), os.path.join(opt.res_dir, name), len(images))


def visualize_multi_cycle(opt, real_B, model, name):
    """test.py:24-31"""
    size = real_B.size()
    images = [one_to_three_channels(img.cpu()).unsqueeze(1) for img in model.generate_multi_cycle(real_B, steps=4)]
    _grid(torch.cat(images, dim=1).view(size[0] * len(images), 3, size[2], size[3]), os.path.join(opt.res_dir, name), len(images))


def visualize_cycle_B_multi(opt, real_B, model, name):
    """test.py:33-46"""
    size = real_B.size()
    z = real_B.new_empty((opt.num_multi, opt.nlatent, 1, 1)).normal_(0, 1).repeat(size[0], 1, 1, 1)
    fake_A, multi_fake_B = model.generate_cycle_B_multi(real_B, z)
    multi = one_to_three_channels(multi_fake_B.cpu()).view(size[0], opt.num_multi, 3, size[2], size[3])
    vis = torch.cat([one_to_three_channels(real_B.cpu()).unsqueeze(1), one_to_three_channels(fake_A.cpu()).unsqueeze(1), multi], 1)
    _grid(vis.view(size[0] * (opt.num_multi + 2), 3, size[2], size[3]), os.path.join(opt.res_dir, name), opt.num_multi + 2)


def visualize_multi(opt, real_A, model, name):
    """test.py:48-60"""
    size = real_A.size()
    z = real_A.new_empty((opt.num_multi, opt.nlatent, 1, 1)).normal_(0, 1).repeat(size[0], 1, 1, 1)
    multi = one_to_three_channels(model.generate_multi(real_A.detach(), z).cpu()).view(size[0], opt.num_multi, 3, size[2], size[3])
    vis = torch.cat([one_to_three_channels(real_A.cpu()).unsqueeze(1), multi], dim=1)
    _grid(vis.view(size[0] * (opt.num_multi + 1), 3, size[2], size[3]), os.path.join(opt.res_dir, name), opt.num_multi + 1)


def visualize_inference(opt, real_A, real_B, model, name):
    """test.py:62-79 (the B row holds the batch's first min(num_multi, batch) samples)"""
    size = real_A.size()
    real_B = real_B[:opt.num_multi]
    k = real_B.size(0)
    multi = one_to_three_channels(model.inference_multi(real_A.detach(), real_B.detach()).cpu()).view(size[0], k, 3, size[2], size[3])
    vis = torch.cat([one_to_three_channels(real_A.cpu()).unsqueeze(1), multi], dim=1).view(size[0] * (k + 1), 3, size[2], size[3])
    vis = torch.cat([torch.ones(1, 3, size[2], size[3]), one_to_three_channels(real_B.cpu()), vis], dim=0)
    _grid(vis, os.path.join(opt.res_dir, name), k + 1)


def sensitivity_to_edge_noise(opt, model, data_B, use_gpu=True):
    """test.py:97-107 (inspired by arXiv:1712.02950): mean |B - rec_B| per sample for eight perturbation levels of fake_A
    -> <res_dir>/noise_sens.npy, shape (8, N)"""
    res = []
    real_B = data_B.cuda() if use_gpu else data_B
    npx = real_B[0].numel()
    with torch.no_grad():
        for std in NOISE_STDS:
            rec_B = model.generate_noisy_cycle(real_B, std)
            s = torch.abs(real_B - rec_B).sum(3).sum(2).sum(1) / npx
            res.append(s.cpu().numpy().tolist())
    np.save(os.path.join(opt.res_dir, 'noise_sens.npy'), np.array(res))
    return np.array(res)


def train_MVGauss_B(dataset):
    """test.py:109-128: per-pixel mean of the batch means, then the mean of the batches' mean squared deviations"""
    b_mean, b_var, n = 0, 0, 0
    for batch in dataset:
        b_mean = b_mean + batch['B'].cuda().mean(0, keepdim=True)
        n += 1
    b_mean = b_mean / n
    for batch in dataset:
        b_var = b_var + ((batch['B'].cuda() - b_mean) ** 2).mean(0, keepdim=True)
    b_var = b_var / n
    return b_mean, b_var


def _nhwc_image(t):
    return ops.ToNHWC.apply(t.contiguous(), True)


def eval_bpp_MVGauss_B(dataset, mu, logvar, dequant_seq=None):
    """test.py:130-141: mean over batches of the batch-mean bpp of dequantised B under N(mu, exp(logvar)) per pixel.
    dequant_seq: test hook, the dequantisation noise of every batch."""
    bpp = []
    mu_c, lv_c = _nhwc_image(mu), _nhwc_image(logvar)
    for i, batch in enumerate(dataset):
        real_B = batch['B'].cuda()
        dequant = dequant_seq[i] if dequant_seq is not None else torch.zeros_like(real_B).uniform_(0, 1. / 127.5)
        real_B = real_B + dequant
        N, npx = real_B.size(0), real_B[0].numel()
        x = _nhwc_image(real_B)
        nll = ops.PixelNLL.apply(x, mu_c.expand_as(x).contiguous(), lv_c, real_B.size(1), "gaussian") + npx * math.log(127.5)
        bpp.append(float(nll.mean(0)) / (npx * math.log(2)))
    return float(np.mean(bpp))


def compute_bpp_MVGauss_B(train_dataset, test_dataset):
    """test.py:143-153 on the given iterators"""
    mvg_mean, mvg_var = train_MVGauss_B(train_dataset)
    return eval_bpp_MVGauss_B(test_dataset, mvg_mean, torch.log(mvg_var + 1e-5))


def train_logvar(dataset, model, epochs=1, use_gpu=True, dequant_seq=None, eps_seq=None, trace=None, verbose=True):
    """test.py:156-196: RMSprop on the per-pixel log-variance of the Laplace likelihood, one update per training batch, with
    the generators frozen: B -> A -> B through the encoder's (or a fixed N(0, 0.01)) code.  The likelihood and its gradient
    w.r.t. logvar_B are ops.PixelNLL.  dequant_seq / eps_seq / trace: test hooks (the two noise draws of batch i, and a list
    receiving (ubo, kld, bpp) of every batch)."""
    shape = (1,) + tuple(dataset.data_B.shape[1:])
    logvar_B = torch.full(shape, math.log(0.01), device="cuda", requires_grad=True)
    opt = torch.optim.RMSprop([logvar_B], lr=1e-2)
    nl, C = model.opt.nlatent, shape[1]
    G, k = model.netG_A_B, 0
    for _ in range(epochs):
        for batch in dataset:
            real_B = batch['B'].cuda() if use_gpu else batch['B']
            N, npx = real_B.size(0), real_B[0].numel()
            dequant = dequant_seq[k] if dequant_seq is not None else torch.zeros_like(real_B).uniform_(0, 1. / 127.5)
            real_B = real_B + dequant
            enc_mu = torch.zeros(N, nl, device=real_B.device)
            enc_logvar = torch.full((N, nl), math.log(0.01), device=real_B.device)
            with torch.no_grad():
                fake_A = model.predict_A(real_B)
                if hasattr(model, 'netE_B'):
                    params = model.predict_enc_params(fake_A, real_B)
                    enc_mu = params[0].reshape(N, nl)
                    if len(params) == 2:
                        enc_logvar = params[1].reshape(N, nl)
                if eps_seq is None:
                    z_B = gauss_reparametrize(enc_mu, enc_logvar)
                else:
                    z_B = eps_seq[k].mul(enc_logvar.mul(0.5).exp()[:, None, :]).add(enc_mu[:, None, :]).clamp(-4., 4.)
                fake_B = G.forward_nhwc(ops.ToNHWC.apply(fake_A, _starts_with_conv(G.model)),
                                        model._z(z_B).reshape(N, -1).contiguous())
            x = ops.ToNHWC.apply(real_B, fake_B.shape[-1] == ops.cimg(C))
            lv = ops.ToNHWC.apply(logvar_B, fake_B.shape[-1] == ops.cimg(C))
            nll = ops.PixelNLL.apply(x, fake_B, lv, C, "laplace")
            kld = kld_std_guss(enc_mu, enc_logvar)
            ubo = (nll + kld) + npx * math.log(127.5)
            ubo_val, kld_val = float(ubo.detach().mean(0)), float(kld.mean(0))
            bpp = ubo_val / (npx * math.log(2.))
            if trace is not None:
                trace.append((ubo_val, kld_val, bpp))
            if verbose:
                print('UBO: %.4f, KLD: %.4f, BPP: %.4f' % (ubo_val, kld_val, bpp))
            opt.zero_grad()
            ubo.mean(0).backward()
            opt.step()
            k += 1
    return logvar_B


def _build(opt):
    if opt.model == 'stoch_cycle_gan':
        return StochCycleGAN(opt, testing=True), False
    if opt.model == 'cycle_gan':
        return StochCycleGAN(opt, ignore_noise=True, testing=True), False
    if opt.model == 'aug_cycle_gan':
        return AugmentedCycleGAN(opt, testing=True), True
    raise NotImplementedError('Specified model is not implemented.')


def _saved_options(expr_dir):
    for name in ('opt.pkl', 'opt.txt'):
        path = os.path.join(expr_dir, name)
        if os.path.exists(path):
            return parse_opt_file(path)
    raise FileNotFoundError("no opt.pkl or opt.txt next to the checkpoint in %s" % expr_dir)


def _merged_options(saved, args):
    """the options of an evaluation: the saved ones of the training run, then everything argparse parsed on top"""
    return argparse.Namespace(**dict(saved, **vars(args)))


def test_model(argv=None):
    """test.py:199-296"""
    args = TestOptions().parse(argv)
    expr_dir = os.path.dirname(os.path.abspath(args.chk_path))
    opt = _merged_options(_saved_options(expr_dir), args)
    opt.expr_dir = expr_dir
    opt.gpu_ids = [i for i in (int(tok) for tok in args.gpu_ids.split(",")) if i >= 0]
    if not opt.gpu_ids or not torch.cuda.is_available():
        raise RuntimeError("dtgan_amd.test runs on the GPU (the HIP kernels); there is no CPU path")
    torch.cuda.set_device(opt.gpu_ids[0])
    opt.gpu_ids = [opt.gpu_ids[0]]
    ops.set_precision(getattr(opt, 'precision', None) or 'bf16x3')

    opt.seed = 12345
    random.seed(opt.seed)
    np.random.seed(opt.seed)
    torch.manual_seed(opt.seed)
    torch.cuda.manual_seed_all(opt.seed)

    opt.res_dir = os.path.join(opt.expr_dir, opt.res_dir)
    os.makedirs(opt.res_dir, exist_ok=True)

    grid_size = getattr(opt, 'grid_size', None)
    if opt.metric in WHOLE_FIELD_METRICS:
        try:
            opt.overlap = check_overlap(opt.overlap, grid_size)
        except ValueError as e:
            raise SystemExit(e.args[0])
    # whole fields for the metrics whose record asks for them; a --native_res run's other metrics score the centre windows it
    # was trained to translate; everything else sees fields resized to grid_size
    native = opt.metric in WHOLE_FIELD_METRICS or bool(getattr(opt, 'native_res', False))
    arrays = load_numpy_data(opt.dataroot, grid_size=grid_size, native_res=native, centre_eval=False)
    if native and opt.metric not in WHOLE_FIELD_METRICS:
        arrays = [centre_windows(a, grid_size) for a in arrays]
    trainA, trainB, devA, devB, testA, testB = arrays = tuple(arrays)
    sub_size = max(int(len(trainA) * 0.2), 1)
    cap = lambda n, b: max(min(b, n), 1)
    train_dataset = UnalignedIterator(trainA[:sub_size], trainB[:sub_size], batch_size=cap(sub_size, 200))
    print('#training images = %d' % len(train_dataset))
    test_dataset = AlignedIterator(testA, testB, batch_size=cap(len(testA), 200))
    print('#test images = %d' % len(test_dataset))
    dev_dataset = AlignedIterator(devA, devB, batch_size=cap(len(devA), 200))
    print('#dev images = %d' % len(dev_dataset))

    model, vis_inf = _build(opt)
    if opt.ema:
        try:
            model.load(opt.chk_path, use_ema=True)
        except KeyError as e:
            raise SystemExit(e.args[0])
        print("evaluating the averaged weights (ema_decay %g)" % getattr(opt, 'ema_decay', 0.0))
    else:
        model.load(opt.chk_path)

    own = {m.name: m for m in METRICS}.get(opt.metric)      # the project's own metrics: one record each, one path for all
    if opt.metric == 'bpp':
        logvar_B = None
        if opt.train_logvar:
            print("training logvar_B on training data...")
            logvar_B = train_logvar(train_dataset, model).detach()
        print("evaluating on test set...")
        t = time.time()
        _, test_bpp_B, _ = eval_ubo_B(test_dataset, model, opt.ubo_steps, logvar_B=logvar_B, verbose=True, compute_l1=True,
                                      vis_path=opt.res_dir, vis_name='test_pred_B')
        print("TEST_BPP_B: %.4f, TIME: %.4f" % (test_bpp_B, time.time() - t))
    elif opt.metric == 'mse':
        dev_mse_A = eval_mse_A(dev_dataset, model)
        test_mse_A = eval_mse_A(test_dataset, model)
        print("DEV_MSE_A: %.4f, TEST_MSE_A: %.4f" % (dev_mse_A, test_mse_A))
    elif opt.metric == 'visual':
        opt.num_multi = 5
        n_vis = 10
        for i, vis_data in enumerate(AlignedIterator(devA, devB, batch_size=cap(len(devA), n_vis))):
            real_A, real_B = vis_data['A'].cuda(), vis_data['B'].cuda()
            prior_z_B = real_A.new_empty((real_A.size(0), opt.nlatent, 1, 1)).normal_(0, 1)
            with torch.no_grad():
                visualize_cycle(opt, real_A, model.generate_cycle(real_A, real_B, prior_z_B), 'cycle_%d.png' % i)
                visualize_multi(opt, real_A, model, 'multi_%d.png' % i)
                visualize_cycle_B_multi(opt, real_B, model, 'cycle_B_multi_%d.png' % i)
                visualize_multi_cycle(opt, real_B, model, 'multi_cycle_%d.png' % i)
                if vis_inf:
                    visualize_inference(opt, real_A, real_B, model, 'inf_%d.png' % i)
        print("VISUAL: %s" % opt.res_dir)
    elif opt.metric == 'noise_sens':
        res = sensitivity_to_edge_noise(opt, model, next(iter(test_dataset))['B'])
        print("NOISE_SENS: %s" % " ".join("%.4f" % v for v in res.mean(1)))
    elif opt.metric == 'mvgauss':
        full_train = UnalignedIterator(trainA, trainB, batch_size=cap(len(trainA), 200))
        print("MVGauss BPP: %.4f" % compute_bpp_MVGauss_B(full_train, test_dataset))
    elif own is not None:
        header, evaluate = own.prepare(opt, model, arrays)
        split = lambda a, b: AlignedIterator(a, b, batch_size=cap(len(a), own.batch_size))
        dev, test = _eval_splits(opt, own.name, evaluate, split(devA, devB), split(testA, testB), header, dtype=own.dtype)
        print(own.report(opt, dev, test))
    else:
        raise NotImplementedError('wrong metric!')
    return opt


if __name__ == "__main__":
    test_model()
