"""Evaluation — Py3 counterpart of /root/reference/augmented_cyclegan/evaluate.py:10-161: B->A MSE and the
variational upper bound / bits-per-pixel on B (RMSprop on per-sample (mu, logvar) THROUGH the generator A -> B).
The reference hard-codes 64*64*3 (evaluate.py:52,104,107); here it is C*H*W of the batch.  Every iterate of the bound
runs on the HIP kernels: the generator forward and its backward to the latent, the pixel likelihood and its gradient
(ops.PixelNLL) and the latent tail — KLD, trace row, RMSprop, next code — in one launch (ops.latent_bound_step).  The
per-iterate numbers stay on the device until the loop ends: one host synchronisation per batch, not two per iterate."""
import math
import os

import numpy as np
import torch

from . import ops
from .model import gauss_reparametrize, kld_std_guss, log_prob_laplace  # noqa: F401  (public helpers, re-exported)
from .modules import _starts_with_conv


def eval_mse_A(dataset, model, use_gpu=True):
    """evaluate.py:10-19"""
    mse_A = []
    for batch in dataset:
        real_A, real_B = batch['A'], batch['B']
        if use_gpu:
            real_A, real_B = real_A.cuda(), real_B.cuda()
        with torch.no_grad():
            pred_A = model.predict_A(real_B)
        mse_A.append(float(((pred_A - real_A) ** 2).mean()))
    return float(np.mean(mse_A))


class _frozen(object):
    """no weight gradients while optimising the latent (the reference lets autograd compute and discard them)"""

    def __init__(self, net):
        self.params = [p for p in net.parameters() if p.requires_grad]

    def __enter__(self):
        for p in self.params:
            p.requires_grad_(False)

    def __exit__(self, *a):
        for p in self.params:
            p.requires_grad_(True)


def variational_ubo(model, real_A, real_B, steps, logvar_B=None, verbose=False, dequant=None, eps_seq=None, trace=None,
                    compute_l1=False, vis_path=None, vis_name=None, vis_batch=25):
    """dequant / eps_seq / trace are test hooks (not in the reference): the dequantisation noise, the reparametrisation
    noise of iterate i (eps_seq[i], shape (N, 1, nlatent)) and a list receiving (ubo, kld, bpp) of every iterate — the
    golden `eval_aug_small_s64` was produced by the reference's model with exactly these draws.  compute_l1: also the
    reference's L1 between the dequantised B and its reconstruction from mu (the code itself under --stoch_enc) at every
    iterate (evaluate.py:75-80, 126-131; printed with verbose, appended to the trace rows).  vis_path / vis_name: a PNG of
    (A, B, prediction) for the first vis_batch samples at iterate 0 and every 100th (evaluate.py:82-87, 133-141)."""
    with _frozen(model.netG_A_B):
        return _variational_ubo(model, real_A, real_B, steps, logvar_B, verbose, dequant, eps_seq, trace, compute_l1, vis_path,
                                vis_name, vis_batch)


def _image(t, Cp):
    """an NCHW image (or logvar plane) in the NHWC storage of a generator output with Cp channels"""
    img = Cp == ops.cimg(t.shape[1])
    if not img and Cp != ops.cpad(t.shape[1]):
        raise ops._lib.AcgError("variational_ubo: a generator output with %d stored channels for %d real ones" % (Cp, t.shape[1]))
    return ops.ToNHWC.apply(t.detach(), img)


def _variational_ubo(model, real_A, real_B, steps, logvar_B=None, verbose=False, dequant=None, eps_seq=None, trace=None,
                     compute_l1=False, vis_path=None, vis_name=None, vis_batch=25):
    """evaluate.py:39-148.  Returns (ubo, kld, bpp) of the LAST evaluated iterate."""
    if (vis_path is None) != (vis_name is None):
        raise ValueError("variational_ubo: vis_path and vis_name go together")
    N, C = real_B.size(0), real_B.size(1)
    nl = model.opt.nlatent
    npx = real_B[0].numel()
    dev = real_A.device
    if dequant is None:
        dequant = torch.zeros_like(real_B).uniform_(0, 1. / 127.5)
    mu = torch.zeros(N, nl, device=dev)
    logvar = torch.full((N, nl), math.log(0.01), device=dev)
    if logvar_B is None:
        logvar_B = torch.full((1,) + tuple(real_B.shape[1:]), math.log(0.01), device=dev)
    if hasattr(model, 'netE_B'):
        with torch.no_grad():
            params = model.predict_enc_params(real_A, real_B)
        mu = params[0].detach().reshape(N, nl).clone()
        if len(params) == 2:
            logvar = params[1].detach().reshape(N, nl).clone()
    stoch_enc = bool(getattr(model.opt, 'stoch_enc', False))
    real_B = real_B + dequant
    G = model.netG_A_B
    x_A = ops.ToNHWC.apply(real_A.detach(), _starts_with_conv(G.model))      # once per batch
    x_B = lv_B = None
    sq_mu, sq_lv = torch.zeros_like(mu), torch.zeros_like(logvar)              # RMSprop square averages (evaluate.py:65)
    rows = torch.zeros((max(steps, 1), 3), device=dev)                       # per iterate: ubo, kld, bpp
    l1 = torch.zeros((max(steps, 1),), device=dev) if compute_l1 else None
    g_mean = torch.full((N,), 1. / N, device=dev)                            # d mean_n(nll_n) / d nll
    z = torch.empty((N, nl), device=dev).requires_grad_(True)                # the code: a leaf the backward stops at

    def draw(i):           # one normal_ of (N, 1, nl) per iterate, as gauss_reparametrize draws it
        e = eps_seq[i] if eps_seq is not None else torch.empty((N, 1, nl), device=dev).normal_()
        return e.reshape(N, nl).float().contiguous()

    def visualize(i):
        with torch.no_grad():
            vz = (z.detach() if stoch_enc else mu)[:vis_batch].reshape(-1, nl, 1, 1)
            vis_B = model.predict_B(real_A[:vis_batch], vz)
        visualize_data([real_A[:vis_batch], real_B[:vis_batch], vis_B], os.path.join(vis_path, '%s_%d.png' % (vis_name, i)))

    eps = draw(0) if steps > 0 else None
    if eps is not None:
        ops.latent_bound_step(mu, logvar, None, None, None, None, None, npx, 0., eps_next=eps, z_next=z.detach())
    if vis_path is not None:
        visualize(0)
    for i in range(steps):
        fake_B = G.forward_nhwc(x_A, model._z(z).reshape(N, -1).contiguous())
        if x_B is None:
            x_B, lv_B = _image(real_B, fake_B.shape[-1]), _image(logvar_B, fake_B.shape[-1])
        nll = ops.PixelNLL.apply(x_B, fake_B, lv_B, C, "laplace")
        if compute_l1:
            if stoch_enc:
                rec_B = fake_B
            else:
                with torch.no_grad():
                    rec_B = G.forward_nhwc(x_A, model._z(mu).contiguous())
            ops.l1_into(x_B, rec_B, C, l1[i])
        z.grad = None
        torch.autograd.backward(nll, g_mean, inputs=[z])
        dz = z.grad if z.grad is not None else torch.zeros_like(mu)
        # the code of the next iterate; after the last one only when a picture shows it (--stoch_enc draws it as the
        # reference does, evaluate.py:123-141) — otherwise the batch makes exactly `steps` draws
        vis_next = vis_path is not None and (i + 1) % 100 == 0
        eps_next = draw(i + 1) if i + 1 < steps or vis_next else None
        ops.latent_bound_step(mu, logvar, sq_mu, sq_lv, eps, dz, nll.detach(), npx, 1e-2, trace_row=rows[i], eps_next=eps_next,
                              z_next=z.detach() if eps_next is not None else None)
        eps = eps_next
        if vis_next:
            visualize(i + 1)
    if steps == 0:
        return float('nan'), float('nan'), float('nan')
    host = rows[:steps].tolist()                                              # the one read of the batch's numbers
    l1_host = l1[:steps].tolist() if compute_l1 else None
    for i, (ubo_val, kld_val, bpp) in enumerate(host):
        if trace is not None:
            trace.append((ubo_val, kld_val, bpp) + ((l1_host[i],) if compute_l1 else ()))
        if verbose:
            res = '[%d] UBO: %.4f, KLD: %.4f, BPP: %.4f' % (i, ubo_val, kld_val, bpp)
            if compute_l1:
                res = '%s, L1: %.4f' % (res, l1_host[i])
            print(res)
    return tuple(host[-1])


def eval_ubo_B(dataset, model, steps=500, use_gpu=True, logvar_B=None, verbose=False, compute_l1=False, vis_path=None,
               vis_name=None, vis_batch=25):
    """evaluate.py:21-37 -> (mean ubo, mean bpp, mean kld)"""
    ubo_B, bpp_B, kld_B = [], [], []
    for batch in dataset:
        real_A, real_B = batch['A'], batch['B']
        if use_gpu:
            real_A, real_B = real_A.cuda(), real_B.cuda()
        ubo, kld, bpp = variational_ubo(model, real_A, real_B, steps, logvar_B, verbose, compute_l1=compute_l1, vis_path=vis_path,
                                        vis_name=vis_name, vis_batch=vis_batch)
        ubo_B.append(ubo); bpp_B.append(bpp); kld_B.append(kld)
    return float(np.mean(ubo_B)), float(np.mean(bpp_B)), float(np.mean(kld_B))


def visualize_data(data, save_path):
    """evaluate.py:163-169: the images of `data` side by side, one sample per row"""
    from .train import save_image_grid
    images = [one_to_three_channels(img.detach().cpu()).unsqueeze(1) for img in data]
    n, _, c, h, w = images[0].shape
    save_image_grid(torch.cat(images, dim=1).view(n * len(images), c, h, w)[:, :3], save_path, nrow=len(images))


def one_to_three_channels(img):
    """evaluate.py:155-161"""
    if img.size(1) == 1:
        z = torch.zeros_like(img)
        return torch.cat((img.float(), z, z), dim=1)
    return img
