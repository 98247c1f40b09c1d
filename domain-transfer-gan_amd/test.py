"""Offline evaluation of a trained checkpoint — Py3 counterpart of /root/reference/augmented_cyclegan/test.py.

    python -m dtgan_amd.test --chk_path <expr_dir>/latest --dataroot <npz dir> --metric bpp|mse|visual|noise_sens|mvgauss|ensemble|spectrum|coherence|fss|translate|field_spectrum|ssim|marginal|minkowski

The saved options of the run are read from opt.pkl next to the checkpoint (or opt.txt, parse_opt_file), the model is rebuilt
with testing=True, seeded with 12345 and loaded.  Metrics (test.py:230-283):
  bpp         the variational bound on B (evaluate.eval_ubo_B, --ubo_steps iterates per test batch of 200), after training the
              per-pixel log-variance logvar_B on the first 20 % of the training data (--train_logvar 1, train_logvar)
  mse         B -> A mean squared error on dev and test
  visual      cycle / multi / cycle-B-multi / multi-cycle (/ inference) grids of every dev batch of 10
  noise_sens  |B - rec_B| per sample after perturbing fake_A with eight noise levels -> <res_dir>/noise_sens.npy
  mvgauss     the multivariate-Gaussian baseline bpp (compute_bpp_MVGauss_B, test.py:123-134; new as a --metric)
  ensemble    (new) the stochastic direction scored as a distribution: --n_samples translations A -> B of every dev and test
              input (model.translate_ensemble), per input the CRPS, its fair form, the MSE of the ensemble mean, the spread
              and the coverage of the outer --quantiles band against the paired B, and the rank histogram of B among the
              members -> <res_dir>/ensemble.npz, and grids of A, B, mean, std and the outer quantiles for the first dev batch
              of 10 (ensemble_0.png)
  spectrum    (new) the variance at every spatial scale: the radially averaged power spectrum (F = fft2 of a channel, |F|^2 / S^2
              averaged over rings of integer wavenumber 0 .. S/2; a HIP FFT, ops.radial_spectrum) of --n_samples translations
              A -> B of every dev and test input and of their per-pixel mean (model.translate_spectrum) against the real B, and
              of B -> A against the real A; split-mean spectra per channel and log-spectral distances in dB over bins
              1 .. S/2 (LSD = sqrt(mean_b (10 log10(p_b / q_b))^2), spectra clamped at 1e-30, the mean over channels), computed
              on the host in float64 -> <res_dir>/spectrum.npz.  Square fields, S a power of two in 16 .. 1024.  No plot
  coherence   (new) whether that variance is in the right place: on the aligned dev and test pairs the cross-spectrum of
              prediction x and truth y per ring (Pxx, Pyy and the co-spectrum Cxy = Re(X conj Y) / S^2; ops.cross_spectrum, one
              transform for both fields) of --n_samples translations A -> B and of their per-pixel mean
              (model.translate_coherence) against the paired B, and of B -> A against the paired A.  The triples are summed
              over the split, then (ops.coherence_summary, float64 on the host) the coherence Cxy^2 / (Pxx Pyy), the signed
              correlation, the error spectrum Pxx + Pyy - 2 Cxy (the MSE split by scale) and the effective resolution k_eff:
              the first ring whose coherence falls below 0.5 (S/2 + 1: none does), printed as its mean over the channels ->
              <res_dir>/coherence.npz.  Sizes as for spectrum.  No plot
  fss         (new) whether threshold exceedances are put close enough: the fractions skill score (Roberts & Lean 2008) per
              channel, threshold and neighbourhood width.  Events are [x >= t]; per odd window n the events around every cell
              are counted (cells outside the domain count 0) for prediction (cf) and truth (co), and the integer triples
              (sum cf^2, sum co^2, sum cf co) come from ops.fss (HIP, exact).  Thresholds: per channel the --fss_quantiles of
              the real training fields (trainB for A -> B, trainA for B -> A; np.quantile in float64, cast to float32), or the
              --fss_thresholds in data units; windows: --fss_windows.  Compared on the aligned dev and test pairs: the
              --n_samples translations A -> B (members_B), the ensemble as a probability (ens_prob_B: the members' summed
              counts, FSS_prob = 2 M sum E co / (sum E^2 + M^2 sum co^2)) and their per-pixel mean (ens_mean_B)
              (model.translate_fss) against the paired B, and B -> A (fake_A) against the paired A.  The triples are summed
              over the split in int64, then (ops.fss_summary, float64 on the host) FSS = 2 sum cf co / (sum cf^2 + sum co^2),
              and from the window 1 the frequency bias, the CSI, the observed base rate f0 and the useful scale: the smallest
              listed window with FSS >= 0.5 + f0 / 2 (0: none).  Printed: FSS at the median listed window and the highest
              threshold, the mean over the channels -> <res_dir>/fss.npz.  Any H x W up to 1024.  No plot
  translate   (new) whole fields at their stored resolution: the data is loaded UNRESIZED, every dev and test field of any
              H x W >= grid_size is cut into overlapping grid_size windows (--overlap pixels shared by neighbours, default
              grid_size // 4), translated window by window and blended at the seams (model.translate_field, --n_samples
              members per field with one code each; model.translate_field_A for B -> A).  Per split, float32:
              <split>_mean_B, <split>_std_B (over the members, unbiased; 0 for one member), <split>_member0_B and
              <split>_fake_A, each (N, C, H, W), with n_samples, window, overlap, origins_y, origins_x ->
              <res_dir>/translate.npz.  Printed: the RMSE of the member mean against the paired B and of fake_A against the
              paired A.  No plot
  field_spectrum (new) spectrum and coherence for those whole fields, in one pass: the data is loaded UNRESIZED as for translate,
              every dev and test field (any H x W >= grid_size, both extents in 16 .. 1024) is translated by the tiled
              model.translate_field (--n_samples members, --overlap), and the members and their per-pixel mean are paired with
              the whole real B, translate_field_A(real B) with the whole real A (model.translate_field_spectrum,
              ops.field_cross_spectrum: Bluestein's chirp-z on the HIP FFT for lengths that are no powers of two).  Rings are
              elliptical: ring b holds the cells of radius L sqrt((fy/H)^2 + (fx/W)^2) rounded to b, L = min(H, W), bins
              0 .. L // 2, "b cycles per L pixels".  The (Pxx, Pyy, Cxy) triples are summed over the split in float64 before
              anything is divided; they carry both families: psd_real_B, psd_members_B, psd_ens_mean_B, psd_real_A, psd_fake_A
              (C, nb) with lsd_B, lsd_mean_B, lsd_A as for spectrum, and sums_k, coh_k, r_k, perr_k, k_eff_k for k in members_B,
              ens_mean_B, fake_A as for coherence, with n_samples, window, overlap, height, width ->
              <res_dir>/field_spectrum.npz.  Seams put power at the window pitch and its multiples, the blend ramp removes
              small-scale variance: neither shows in translate's RMSE.  Printed: LSD_B, LSD_A and the channel mean of k_eff
              of the members.  No plot
  ssim        (new) the local structure: the structural similarity (Wang et al. 2004; 11 x 11 Gaussian window, sigma 1.5,
              data range 2, valid positions; ops.ssim, HIP) on the aligned dev and test pairs, of the --n_samples translations
              A -> B (members_B) and of their per-pixel mean (ens_mean_B) (model.translate_ssim) against the paired B, and
              of B -> A (fake_A) against the paired A.  Per comparison k, float64: ssim_k and cs_k (C,), the split means of
              the mean S and of the mean contrast-structure factor cs, and ssim_k_per_input, cs_k_per_input (N, C), the
              members averaged per input -> <res_dir>/ssim.npz.  The mean of an ensemble is smoother than its members: a
              higher luminance term, a lower cs; the file shows both.  Printed: the channel means.  11 <= H, W <= 1024.
              No plot
  marginal    (new) whether the values are right, wherever they lie: every field is sorted on the device (ops.field_sort, HIP)
              and from the sorted fields (ops.sorted_scores, one launch) come, per channel, the 1-Wasserstein distance w1 =
              mean_k |s_x[k] - s_y[k]| and the squared 2-Wasserstein distance w2sq = mean_k (s_x[k] - s_y[k])^2 of a field's
              value distribution against that of its paired truth (in double), its quantiles at the --marg_levels
              (np.quantile, method "linear") and its exact counts of values below the edges: per channel the quantiles k / B,
              k = 1 .. B - 1, B = --marg_bins, of the real training fields (trainB for A -> B, trainA for B -> A; np.quantile in
              float64, cast to float32).  Compared on the aligned dev and test pairs: the --n_samples translations A -> B
              (members_B) and their per-pixel mean (ens_mean_B) (model.translate_marginal) against the paired B, and B -> A
              (fake_A) against the paired A.  Per comparison k: w1_k, w2sq_k (C,), the split means, and w1_k_per_input,
              w2sq_k_per_input (N, C), the members averaged per input; q_k (C, L), the mean over the fields of their
              quantiles (q_real_B, q_real_A: of the truths: a Q-Q curve); below_k (C, E) int64, the counts summed over inputs
              and members, in cells_k cells (below_real_*, cells_real_*: of the truths), and from them (ops.marginal_summary)
              the pooled distribution function cdf_k at the edges and ks_k (C,), its Kolmogorov-Smirnov distance to that of
              the truths, with levels, edges_B, edges_A -> <res_dir>/marginal.npz.  P - below is the count of fss's events.
              Printed: the channel means of w1 and ks.  H W <= 2^20.  No plot
  minkowski   (new) the shape of the threshold exceedances, which none of the above sees: the Minkowski functionals of the
              excursion sets {x >= t} - area, perimeter and the Euler characteristic (components minus holes, for 4- and for
              8-connectivity) - as curves over the thresholds t: per channel the quantiles k / B, k = 1 .. B - 1, B =
              --mink_bins, of the real training fields (trainB for A -> B, trainA for B -> A; marginal_edges).  ops.minkowski
              (HIP, exact integers, one pass over a field for all thresholds) gives the counts (nF, nE1, nE2, nV1, nV4) of
              cells, edges and vertices touching / inside each set; they are summed in int64 over five SETS of fields - the
              --n_samples translations A -> B (members_B), their per-pixel means (ens_mean_B) (model.translate_minkowski),
              B -> A (fake_A) and the real fields of both domains (real_B, real_A) - before anything is divided.  Unpaired:
              sets are compared with sets, as the model is trained.  Per set k: counts_k (C, T, 5) int64, cells_k, and
              (ops.minkowski_summary, float64) area_k = nF, perimeter_k = nE1 - nE2, euler8_k = nV1 - nE1 + nF, euler4_k =
              nF - nE2 + nV4 (C, T), each also per cell (*_density_k); per translated set k against the real set of its
              domain (ops.minkowski_distance): dist_area_k, dist_perimeter_k, dist_euler4_k, dist_euler8_k (C,), the mean
              over the thresholds of the absolute difference of the densities, with n_samples, bins, thresholds_B,
              thresholds_A -> <res_dir>/minkowski.npz.  A blobby, a filamentary and a speckled field can share marginal,
              spectrum and FSS and differ here; the mean of an ensemble loses objects and boundary.  Printed per split: the
              four distances of members_B, ens_mean_B and fake_A, the channel means.  1 <= H, W <= 1024.  No plot

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
from .evaluate import eval_mse_A, eval_ubo_B, one_to_three_channels
from .model import AugmentedCycleGAN, StochCycleGAN, gauss_reparametrize, kld_std_guss
from .modules import _starts_with_conv
from .options import TestOptions, check_overlap
from .train import save_image_grid

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


def _read_back(tensors):
    """device tensors of one dtype -> host arrays of their shapes, through ONE device->host copy"""
    tensors = list(tensors)
    host = torch.cat([t.reshape(-1) for t in tensors]).cpu().numpy()
    ends = np.cumsum([t.numel() for t in tensors])
    return [host[e - t.numel():e].reshape(tuple(t.shape)) for e, t in zip(ends, tensors)]


ENSEMBLE_SCORES = ('crps', 'crps_fair', 'mse_mean', 'spread', 'coverage')


def eval_ensemble_B(dataset, model, n_samples, quantiles, use_gpu=True):
    """the per-input ensemble scores of A -> B on an aligned split (model.translate_ensemble, one read of the numbers per
    batch) -> ({score: (N,) array for every input}, rank histogram pooled over the split (n_samples + 1,))"""
    per, hist = {k: [] for k in ENSEMBLE_SCORES}, np.zeros(n_samples + 1, dtype=np.int64)
    for batch in dataset:
        real_A, real_B = batch['A'], batch['B']
        if use_gpu:
            real_A, real_B = real_A.cuda(), real_B.cuda()
        r = model.translate_ensemble(real_A, n_samples, real_B=real_B, quantiles=quantiles)
        *scores, ranks = _read_back([r[k].double() for k in ENSEMBLE_SCORES + ('rank_hist',)])
        for k, v in zip(ENSEMBLE_SCORES, scores):
            per[k].append(v)
        hist += ranks.sum(0).astype(np.int64)
    return {k: np.concatenate(v) for k, v in per.items()}, hist


def visualize_ensemble(opt, real_A, real_B, model, name):
    """rows A, B, ensemble mean, std (scaled to the image range by the grid's largest value), lowest and highest quantile;
    one column per input"""
    r = model.translate_ensemble(real_A, opt.n_samples, quantiles=opt.quantiles)
    std = r['std']
    std = std * (2. / max(float(std.max()), 1e-12)) - 1.
    rows = [real_A, real_B, r['mean'], std, r['quantiles'][:, 0], r['quantiles'][:, -1]]
    _grid(torch.cat([one_to_three_channels(x.detach().cpu()) for x in rows], 0), os.path.join(opt.res_dir, name), real_A.size(0))


def log_spectral_distance(p, q):
    """(..., C, nb) spectra -> (...,) float64: sqrt(mean over bins 1 .. S/2 of (10 log10(p / q))^2) in dB, both clamped at
    1e-30, averaged over the channels"""
    p = np.maximum(np.asarray(p, dtype=np.float64)[..., 1:], 1e-30)
    q = np.maximum(np.asarray(q, dtype=np.float64)[..., 1:], 1e-30)
    return np.sqrt(np.mean((10.0 * np.log10(p / q)) ** 2, axis=-1)).mean(axis=-1)


def eval_spectrum(dataset, model, n_samples, use_gpu=True):
    """radially averaged power spectra on an aligned split, one read of the bin arrays per batch.  A -> B: n_samples members
    per input and their ensemble mean (model.translate_spectrum) against the real B; B -> A: predict_A against the real A.
    -> dict: psd_real_B, psd_members_B (over inputs and members), psd_ens_mean_B, psd_real_A, psd_fake_A: split means, (C, nb)
    float64; lsd_B, lsd_mean_B, lsd_A: the distances of those means; lsd_B_per_input (N,): every input's member-mean
    spectrum against its own paired B"""
    keys = ('members', 'ens_mean', 'target', 'real_A', 'fake_A')
    parts = {k: [] for k in keys}
    for batch in dataset:
        real_A, real_B = batch['A'], batch['B']
        if use_gpu:
            real_A, real_B = real_A.cuda(), real_B.cuda()
        r = model.translate_spectrum(real_A, n_samples, real_B=real_B)
        with torch.no_grad():
            r['fake_A'] = ops.radial_spectrum(model.predict_A(real_B), real_A.size(1), "nchw")
        r['real_A'] = ops.radial_spectrum(real_A, real_A.size(1), "nchw")
        for k, v in zip(keys, _read_back([r[k] for k in keys])):
            parts[k].append(v.astype(np.float64))
    p = {k: np.concatenate(v) for k, v in parts.items()}
    res = dict(psd_real_B=p['target'].mean(0), psd_members_B=p['members'].mean((0, 1)), psd_ens_mean_B=p['ens_mean'].mean(0),
               psd_real_A=p['real_A'].mean(0), psd_fake_A=p['fake_A'].mean(0))
    res['lsd_B'] = float(log_spectral_distance(res['psd_members_B'], res['psd_real_B']))
    res['lsd_mean_B'] = float(log_spectral_distance(res['psd_ens_mean_B'], res['psd_real_B']))
    res['lsd_A'] = float(log_spectral_distance(res['psd_fake_A'], res['psd_real_A']))
    res['lsd_B_per_input'] = log_spectral_distance(p['members'].mean(1), p['target'])
    return res


COHERENCE_PAIRS = ('members_B', 'ens_mean_B', 'fake_A')


def _coherence_entries(sums, pairs):
    """per comparison k of COHERENCE_PAIRS: the summed triples sums_k and ops.coherence_summary of them, perr_k per pair"""
    res = {}
    for k in COHERENCE_PAIRS:
        res['sums_' + k] = sums[k]
        summary = ops.coherence_summary(sums[k])
        summary['perr'] = summary['perr'] / pairs[k]
        res.update(('%s_%s' % (name, k), v) for name, v in summary.items())
    return res


def eval_coherence(dataset, model, n_samples, use_gpu=True):
    """paired cross-spectra on an aligned split, one read of the bin arrays per batch.  A -> B: n_samples members per input
    and their ensemble mean (model.translate_coherence) against the paired real B; B -> A: predict_A against the paired real
    A.  The (pxx, pyy, cxy) triples of every comparison are summed over the split (over the members too) before anything is
    divided: one pair's ring-wise coherence is noisy where a ring has few cells.  -> dict, per comparison k of
    COHERENCE_PAIRS: sums_k (C, 3, nb) float64 and coh_k, r_k, perr_k (C, nb), k_eff_k (C,) of ops.coherence_summary; perr_k
    is the mean error spectrum per pair (the summed one over the number of pairs)"""
    sums = {k: 0.0 for k in COHERENCE_PAIRS}
    pairs = {k: 0 for k in COHERENCE_PAIRS}
    for batch in dataset:
        real_A, real_B = batch['A'], batch['B']
        if use_gpu:
            real_A, real_B = real_A.cuda(), real_B.cuda()
        r = model.translate_coherence(real_A, n_samples, real_B)
        with torch.no_grad():
            fake_A = ops.cross_spectrum(model.predict_A(real_B), real_A, real_A.size(1), "nchw", "nchw")
        parts = (r['members'].flatten(0, 1), r['ens_mean'], fake_A)
        for k, v in zip(COHERENCE_PAIRS, _read_back(parts)):
            sums[k] = sums[k] + v.astype(np.float64).sum(0)
            pairs[k] += v.shape[0]
    return _coherence_entries(sums, pairs)


SSIM_PAIRS = ('members_B', 'ens_mean_B', 'fake_A')


def eval_ssim(dataset, model, n_samples, use_gpu=True):
    """structural similarity on an aligned split, one read of the (S, cs) pairs per batch.  A -> B: n_samples members per
    input and their ensemble mean (model.translate_ssim) against the paired real B; B -> A: predict_A against the paired real
    A.  -> dict, per comparison k of SSIM_PAIRS, float64: ssim_k, cs_k (C,), the means over the split (and the members), and
    ssim_k_per_input, cs_k_per_input (N, C), the members averaged per input"""
    parts = {k: [] for k in SSIM_PAIRS}
    for batch in dataset:
        real_A, real_B = batch['A'], batch['B']
        if use_gpu:
            real_A, real_B = real_A.cuda(), real_B.cuda()
        r = model.translate_ssim(real_A, n_samples, real_B)
        with torch.no_grad():
            fake_A = ops.ssim(model.predict_A(real_B), real_A, real_A.size(1), "nchw", "nchw")
        got = _read_back((r['members'], r['ens_mean'], fake_A))
        parts['members_B'].append(got[0].astype(np.float64).mean(1))
        parts['ens_mean_B'].append(got[1].astype(np.float64))
        parts['fake_A'].append(got[2].astype(np.float64))
    res = {}
    for k in SSIM_PAIRS:
        v = np.concatenate(parts[k])                               # (N, C, 2)
        res['ssim_' + k], res['cs_' + k] = v[..., 0].mean(0), v[..., 1].mean(0)
        res['ssim_%s_per_input' % k], res['cs_%s_per_input' % k] = v[..., 0], v[..., 1]
    return res


MARGINAL_PAIRS = ('members_B', 'ens_mean_B', 'fake_A')


def marginal_edges(train, bins):
    """the edges the distribution functions of one domain are compared at -> (C, bins - 1) float32: per channel the quantiles
    k / bins, k = 1 .. bins - 1, of its real training fields (N, C, H, W), np.quantile in float64 as fss_thresholds takes its
    thresholds.  Repeated edges (a field with mass at one value) are kept: every count is independent"""
    bins = int(bins)
    if not 2 <= bins <= ops.MARG_MAX_EDGES + 1:
        raise ValueError("marginal_edges: bins must lie in 2..%d (got %d)" % (ops.MARG_MAX_EDGES + 1, bins))
    train = np.asarray(train)
    C = train.shape[1]
    x = train.astype(np.float64).transpose(1, 0, 2, 3).reshape(C, -1)
    return np.quantile(x, np.arange(1, bins, dtype=np.float64) / bins, axis=1).T.astype(np.float32)


def _marginal_entries(parts, real):
    """eval_marginal's result from what its batches gave.  parts[k], per comparison k of MARGINAL_PAIRS: lists of w (n, C, 2)
    float64 (the members averaged per input), q (C, L) float64 sums over the fields, below (C, E) int64 sums, and the numbers
    of fields and of cells they run over; real['B'], real['A']: q, below, fields, cells of the paired real fields of that
    direction"""
    res = {}
    for k in MARGINAL_PAIRS:
        p, r = parts[k], real[k[-1]]
        w = np.concatenate(p['w'])                                 # (N, C, 2)
        res['w1_' + k], res['w2sq_' + k] = w[..., 0].mean(0), w[..., 1].mean(0)
        res['w1_%s_per_input' % k], res['w2sq_%s_per_input' % k] = w[..., 0], w[..., 1]
        res['q_' + k] = p['q'] / float(p['fields'])
        res['below_' + k], res['cells_' + k] = np.asarray(p['below'], dtype=np.int64), np.int64(p['cells'])
        summary = ops.marginal_summary(p['below'], p['cells'], r['below'], r['cells'])
        res['cdf_' + k], res['ks_' + k] = summary['cdf'], summary['ks']
    for d in ('B', 'A'):
        r = real[d]
        res['q_real_' + d] = r['q'] / float(r['fields'])
        res['below_real_' + d], res['cells_real_' + d] = np.asarray(r['below'], dtype=np.int64), np.int64(r['cells'])
    return res


def eval_marginal(dataset, model, n_samples, levels, edges_B, edges_A, use_gpu=True):
    """the value distributions on an aligned split, one read of the scores per batch.  A -> B: n_samples members per input and
    their ensemble mean against the paired real B, and the real B itself (model.translate_marginal); B -> A: predict_A against
    the paired real A, and the real A itself (ops.marginal_scores).  -> dict, per comparison k of MARGINAL_PAIRS: w1_k, w2sq_k
    (C,) float64, the split means of the per-field Wasserstein distances, with w1_k_per_input, w2sq_k_per_input (N, C), the
    members averaged per input; q_k (C, L), the mean over the fields of their quantiles; below_k (C, E) int64, the counts
    below the edges summed over inputs and members, in cells_k cells; cdf_k (C, E) and ks_k (C,) of ops.marginal_summary
    against the real fields of that direction.  For those: q_real_B, q_real_A, below_real_B, below_real_A, cells_real_B,
    cells_real_A"""
    zero = lambda: dict(w=[], q=0.0, below=0, fields=0, cells=0)
    parts, real = {k: zero() for k in MARGINAL_PAIRS}, {d: zero() for d in ('B', 'A')}
    e_B = e_A = None

    def add(acc, q, below, cells_per_field):
        """q (..., C, L) float32 and below (..., C, E) int32 of some fields, summed over the leading axes in float64 / int64"""
        q, below = q.reshape((-1,) + q.shape[-2:]), below.reshape((-1,) + below.shape[-2:])
        acc['q'] = acc['q'] + q.astype(np.float64).sum(0)
        acc['below'] = acc['below'] + below.sum(0, dtype=np.int64)
        acc['fields'] += q.shape[0]
        acc['cells'] += q.shape[0] * cells_per_field

    for batch in dataset:
        real_A, real_B = batch['A'], batch['B']
        if use_gpu:
            real_A, real_B = real_A.cuda(), real_B.cuda()
        if e_B is None:
            e_B = torch.from_numpy(np.ascontiguousarray(edges_B)).to(real_B.device)
            e_A = torch.from_numpy(np.ascontiguousarray(edges_A)).to(real_A.device)
        r = model.translate_marginal(real_A, n_samples, real_B, levels, e_B)
        CA = real_A.size(1)
        with torch.no_grad():
            fake_A = ops.marginal_scores(model.predict_A(real_B), real_A, CA, "nchw", "nchw", levels, e_A)
        tgt_A = ops.marginal_scores(real_A, None, CA, "nchw", None, levels, e_A)
        groups = (r['members'], r['ens_mean'], fake_A)
        # one copy: the doubles as they are, the float32 quantiles and the int32 counts widened exactly
        host = _read_back([g['w'] for g in groups]
                          + [t[k].double() for t in groups + (r['target'], tgt_A) for k in ('q', 'below')])
        w, rest = host[:3], host[3:]
        cells = (real_B.size(2) * real_B.size(3), real_B.size(2) * real_B.size(3), real_A.size(2) * real_A.size(3))
        for i, k in enumerate(MARGINAL_PAIRS):
            parts[k]['w'].append(w[i].mean(1) if k == 'members_B' else w[i])
            add(parts[k], rest[2 * i], rest[2 * i + 1].astype(np.int64), cells[i])
        add(real['B'], rest[6], rest[7].astype(np.int64), cells[0])
        add(real['A'], rest[8], rest[9].astype(np.int64), cells[2])
    return _marginal_entries(parts, real)


FSS_PAIRS = ('members_B', 'ens_prob_B', 'ens_mean_B', 'fake_A')


def fss_thresholds(train, quantiles, explicit=None):
    """the event thresholds of one domain -> (C, T) float32: the explicit values for every channel, else per channel the
    quantile levels of its real training fields (N, C, H, W), np.quantile in float64"""
    train = np.asarray(train)
    C = train.shape[1]
    if explicit is not None:
        return np.tile(np.asarray(explicit, dtype=np.float32)[None, :], (C, 1))
    x = train.astype(np.float64).transpose(1, 0, 2, 3).reshape(C, -1)
    return np.quantile(x, np.asarray(quantiles, dtype=np.float64), axis=1).T.astype(np.float32)


def eval_fss(dataset, model, n_samples, thresholds_B, thresholds_A, windows, use_gpu=True):
    """fractions-skill-score triples on an aligned split, one read of the sums per batch.  A -> B: n_samples members per
    input, the ensemble as a probability and the ensemble mean (model.translate_fss) against the paired real B; B -> A:
    predict_A against the paired real A.  The int64 triples of every comparison are summed over the split (over the members
    too) before anything is divided.  -> dict, per comparison k of FSS_PAIRS: sums_k (C, T, nw, 3) int64 and fss_k (C, T, nw),
    bias_k, csi_k, base_rate_k (C, T), useful_scale_k (C, T) int64 of ops.fss_summary (ens_prob_B with members=n_samples)"""
    sums = {k: 0 for k in FSS_PAIRS}
    cells = {k: 0 for k in FSS_PAIRS}
    thr_B = thr_A = None
    for batch in dataset:
        real_A, real_B = batch['A'], batch['B']
        if use_gpu:
            real_A, real_B = real_A.cuda(), real_B.cuda()
        if thr_B is None:
            thr_B = torch.from_numpy(np.ascontiguousarray(thresholds_B)).to(real_B.device)
            thr_A = torch.from_numpy(np.ascontiguousarray(thresholds_A)).to(real_A.device)
        r = model.translate_fss(real_A, n_samples, real_B, thr_B, windows)
        with torch.no_grad():
            fake_A = ops.fss(model.predict_A(real_B), real_A, real_A.size(1), "nchw", "nchw", thr_A, windows)
        parts = (r['members'].flatten(0, 1), r['ens_prob'], r['ens_mean'], fake_A)
        for k, v in zip(FSS_PAIRS, _read_back(parts)):
            sums[k] = sums[k] + v.sum(0, dtype=np.int64)
            cells[k] += v.shape[0] * real_B.size(2) * real_B.size(3)
    res = {}
    for k in FSS_PAIRS:
        res['sums_' + k] = np.asarray(sums[k], dtype=np.int64)
        summary = ops.fss_summary(sums[k], windows, cells[k], members=n_samples if k == 'ens_prob_B' else 1)
        res.update(('%s_%s' % (name, k), v) for name, v in summary.items())
    return res


MINKOWSKI_SETS = ('members_B', 'ens_mean_B', 'fake_A', 'real_B', 'real_A')
MINKOWSKI_PAIRS = (('members_B', 'real_B'), ('ens_mean_B', 'real_B'), ('fake_A', 'real_A'))


def eval_minkowski(dataset, model, n_samples, thr_B, thr_A, use_gpu=True):
    """the shape of the excursion sets on a split, one read of the counts per batch.  The counts of ops.minkowski, at the
    thresholds thr_B (C_B, T) in domain B and thr_A (C_A, T) in domain A, are summed in int64 over the fields of five sets:
    the n_samples translations A -> B of every input (members_B) and their per-pixel means (ens_mean_B)
    (model.translate_minkowski), B -> A (fake_A, predict_A), and the real fields of both domains through the same kernel
    (real_B, real_A).  Unpaired: the sets are compared as sets.  -> dict, per set k of MINKOWSKI_SETS: counts_k (C, T, 5)
    int64, cells_k int64 and the float64 (C, T) arrays of ops.minkowski_summary, area_k, perimeter_k, euler4_k, euler8_k and
    the same per cell under *_density_k; per translated set k, against the real set of its domain (MINKOWSKI_PAIRS):
    dist_area_k, dist_perimeter_k, dist_euler4_k, dist_euler8_k (C,) of ops.minkowski_distance"""
    sums = {k: 0 for k in MINKOWSKI_SETS}
    cells = {k: 0 for k in MINKOWSKI_SETS}
    t_B = t_A = None
    for batch in dataset:
        real_A, real_B = batch['A'], batch['B']
        if use_gpu:
            real_A, real_B = real_A.cuda(), real_B.cuda()
        if t_B is None:
            t_B = torch.from_numpy(ops.check_thresholds(thr_B, real_B.size(1))).to(real_B.device)
            t_A = torch.from_numpy(ops.check_thresholds(thr_A, real_A.size(1))).to(real_A.device)
        r = model.translate_minkowski(real_A, n_samples, t_B)
        CA, CB = real_A.size(1), real_B.size(1)
        with torch.no_grad():
            fake_A = ops.minkowski(model.predict_A(real_B), CA, "nchw", t_A)
        parts = (r['members'].flatten(0, 1), r['ens_mean'], fake_A, ops.minkowski(real_B, CB, "nchw", t_B),
                 ops.minkowski(real_A, CA, "nchw", t_A))
        fields = [p.size(0) for p in parts]
        for k, n, v in zip(MINKOWSKI_SETS, fields, _read_back([p.sum(0).reshape(-1) for p in parts])):
            side = real_A if k.endswith('_A') else real_B
            sums[k] = sums[k] + v.reshape(side.size(1), -1, 5).astype(np.int64)
            cells[k] += n * side.size(2) * side.size(3)
    res, summary = {}, {}
    for k in MINKOWSKI_SETS:
        res['counts_' + k], res['cells_' + k] = np.asarray(sums[k], dtype=np.int64), np.int64(cells[k])
        summary[k] = ops.minkowski_summary(sums[k], cells[k])
        res.update(('%s_%s' % (name, k), v) for name, v in summary[k].items())
    for k, real in MINKOWSKI_PAIRS:
        res.update(('dist_%s_%s' % (name, k), v) for name, v in ops.minkowski_distance(summary[k], summary[real]).items())
    return res


def eval_translate(dataset, model, n_samples, overlap, use_gpu=True):
    """whole-field translation of an aligned split at its stored resolution (model.translate_field, translate_field_A), one
    read per batch -> dict of float32 arrays (N, C, H, W): mean_B and std_B over the members (torch on the canvases; std
    unbiased, 0 for one member), member0_B, fake_A; and the scalars rmse_mean_B, rmse_A against the paired real fields, pooled
    over the split in float64"""
    keys = ('mean_B', 'std_B', 'member0_B', 'fake_A')
    parts = {k: [] for k in keys}
    sse, cells = np.zeros(2), np.zeros(2)
    for batch in dataset:
        real_A, real_B = batch['A'], batch['B']
        if use_gpu:
            real_A, real_B = real_A.cuda(), real_B.cuda()
        fake_B = model.translate_field(real_A, n_samples, overlap=overlap)
        r = dict(mean_B=fake_B.mean(1), std_B=fake_B.std(1) if n_samples > 1 else torch.zeros_like(fake_B[:, 0]),
                 member0_B=fake_B[:, 0], fake_A=model.translate_field_A(real_B, overlap=overlap))
        err = torch.stack([(r['mean_B'] - real_B).double().pow(2).sum(), (r['fake_A'] - real_A).double().pow(2).sum()])
        *maps, err = _read_back([r[k].double() for k in keys] + [err])
        for k, v in zip(keys, maps):
            parts[k].append(v.astype(np.float32))
        sse += err
        cells += (real_B.numel(), real_A.numel())
    res = {k: np.concatenate(v) for k, v in parts.items()}
    res['rmse_mean_B'], res['rmse_A'] = np.sqrt(sse / cells)
    return res


def eval_field_spectrum(dataset, model, n_samples, overlap, use_gpu=True):
    """whole-field cross-spectra of an aligned split at its stored resolution, one read of the bin arrays per batch.  A -> B:
    n_samples tiled translations per field and their per-pixel mean (model.translate_field_spectrum) against the paired whole
    real B; B -> A: translate_field_A against the paired whole real A.  The (pxx, pyy, cxy) triples of every comparison are
    summed over the split (over the members too) in float64 before anything is divided.  -> dict: per comparison k of
    COHERENCE_PAIRS what eval_coherence gives (sums_k, coh_k, r_k, perr_k, k_eff_k); the split-mean spectra the triples carry,
    (C, nb) float64: psd_members_B, psd_ens_mean_B, psd_fake_A (pxx) and psd_real_B, psd_real_A (pyy, once per input); and the
    distances lsd_B, lsd_mean_B, lsd_A of those means"""
    sums = {k: 0.0 for k in COHERENCE_PAIRS}
    pairs = {k: 0 for k in COHERENCE_PAIRS}
    for batch in dataset:
        real_A, real_B = batch['A'], batch['B']
        if use_gpu:
            real_A, real_B = real_A.cuda(), real_B.cuda()
        r = model.translate_field_spectrum(real_A, n_samples, real_B, overlap=overlap)
        fake_A = ops.field_cross_spectrum(model.translate_field_A(real_B, overlap=overlap), real_A, real_A.size(1), "nchw", "nchw")
        parts = (r['members'].flatten(0, 1), r['ens_mean'], fake_A)
        for k, v in zip(COHERENCE_PAIRS, _read_back(parts)):
            sums[k] = sums[k] + v.astype(np.float64).sum(0)
            pairs[k] += v.shape[0]
    res = _coherence_entries(sums, pairs)
    for k in COHERENCE_PAIRS:
        res['psd_' + k] = sums[k][:, 0] / pairs[k]
    res['psd_real_B'] = sums['ens_mean_B'][:, 1] / pairs['ens_mean_B']
    res['psd_real_A'] = sums['fake_A'][:, 1] / pairs['fake_A']
    res['lsd_B'] = float(log_spectral_distance(res['psd_members_B'], res['psd_real_B']))
    res['lsd_mean_B'] = float(log_spectral_distance(res['psd_ens_mean_B'], res['psd_real_B']))
    res['lsd_A'] = float(log_spectral_distance(res['psd_fake_A'], res['psd_real_A']))
    return res


WHOLE_FIELD_METRICS = ('translate', 'field_spectrum')     # load the fields unresized and take --overlap


def _chan_mean(v):
    v = np.asarray(v, dtype=np.float64)
    return float(np.nanmean(v)) if np.isfinite(v).any() else float('nan')


def _pooled_spread(spread):
    return float(np.sqrt(np.mean(np.square(spread))))


def _eval_splits(opt, metric, evaluate, dev_dataset, test_dataset, header, dtype=None):
    """What the ensemble metrics share: evaluate(dataset) -> dict on dev, then on test, from the evaluator's seed alone (so
    the codes of dev, then test, follow from it), both written under dev_ / test_ prefixes on top of the metric's `header`
    entries to <res_dir>/<metric>.npz (dtype: what every value is cast to, None: as it comes) -> (dev, test)"""
    torch.manual_seed(opt.seed)
    dev, test = evaluate(dev_dataset), evaluate(test_dataset)
    arrays = dict(header)
    for split, res in (('dev', dev), ('test', test)):
        arrays.update(('%s_%s' % (split, k), np.asarray(v, dtype=dtype)) for k, v in res.items())
    np.savez(os.path.join(opt.res_dir, metric + '.npz'), **arrays)
    return dev, test


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


def test_model(argv=None):
    """test.py:199-296"""
    args = TestOptions().parse(argv)
    opt = argparse.Namespace(**vars(args))
    expr_dir = os.path.dirname(os.path.abspath(args.chk_path))
    opt.__dict__.update(_saved_options(expr_dir))
    for k in ('chk_path', 'res_dir', 'train_logvar', 'dataroot', 'metric', 'ubo_steps', 'n_samples', 'quantiles', 'fss_quantiles', 'fss_thresholds',
              'fss_windows', 'ema', 'overlap', 'marg_levels', 'marg_bins', 'mink_bins'):
        setattr(opt, k, getattr(args, k))
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
    # whole fields for --metric translate and field_spectrum; a --native_res run's other metrics score the centre windows it
    # was trained to translate; everything else sees fields resized to grid_size
    native = opt.metric in WHOLE_FIELD_METRICS or bool(getattr(opt, 'native_res', False))
    arrays = load_numpy_data(opt.dataroot, grid_size=grid_size, native_res=native, centre_eval=False)
    if native and opt.metric not in WHOLE_FIELD_METRICS:
        arrays = [centre_windows(a, grid_size) for a in arrays]
    trainA, trainB, devA, devB, testA, testB = arrays
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
    elif opt.metric == 'ensemble':
        def scored(dataset):
            scores, hist = eval_ensemble_B(dataset, model, opt.n_samples, opt.quantiles)
            return dict(scores, rank_hist=hist)
        dev, test = _eval_splits(opt, 'ensemble', scored, dev_dataset, test_dataset,
                                 dict(n_samples=np.int64(opt.n_samples), quantiles=np.array(opt.quantiles, dtype=np.float64)))
        vis = next(iter(AlignedIterator(devA, devB, batch_size=cap(len(devA), 10))))
        visualize_ensemble(opt, vis['A'].cuda(), vis['B'].cuda(), model, 'ensemble_0.png')
        print("DEV_CRPS_B: %.4f, TEST_CRPS_B: %.4f, TEST_MSE_MEAN_B: %.4f, TEST_SPREAD_B: %.4f, TEST_COVERAGE_B: %.4f"
              % (dev['crps'].mean(), test['crps'].mean(), test['mse_mean'].mean(), _pooled_spread(test['spread']),
                 test['coverage'].mean()))
    elif opt.metric == 'spectrum':
        dev, test = _eval_splits(opt, 'spectrum', lambda d: eval_spectrum(d, model, opt.n_samples), dev_dataset, test_dataset,
                                 dict(n_samples=np.int64(opt.n_samples), bin_counts=ops.spectrum_bins(devA.shape[-1])),
                                 dtype=np.float64)
        print("DEV_LSD_B: %.4f, TEST_LSD_B: %.4f, TEST_LSD_MEAN_B: %.4f, TEST_LSD_A: %.4f"
              % (dev['lsd_B'], test['lsd_B'], test['lsd_mean_B'], test['lsd_A']))
    elif opt.metric == 'coherence':
        dev, test = _eval_splits(opt, 'coherence', lambda d: eval_coherence(d, model, opt.n_samples), dev_dataset, test_dataset,
                                 dict(n_samples=np.int64(opt.n_samples), bin_counts=ops.spectrum_bins(devA.shape[-1])))
        print("DEV_KEFF_B: %.4f, TEST_KEFF_B: %.4f, TEST_KEFF_MEAN_B: %.4f, TEST_KEFF_A: %.4f, TEST_COH_B: %.4f"
              % (dev['k_eff_members_B'].mean(), test['k_eff_members_B'].mean(), test['k_eff_ens_mean_B'].mean(),
                 test['k_eff_fake_A'].mean(), test['coh_members_B'][:, 1:].mean()))
    elif opt.metric == 'fss':
        thr_B = fss_thresholds(trainB, opt.fss_quantiles, opt.fss_thresholds)     # once: dev and test share the climatology
        thr_A = fss_thresholds(trainA, opt.fss_quantiles, opt.fss_thresholds)
        win = tuple(opt.fss_windows)
        header = dict(n_samples=np.int64(opt.n_samples), windows=np.array(win, dtype=np.int64), thresholds_B=thr_B, thresholds_A=thr_A)
        dev, test = _eval_splits(opt, 'fss', lambda d: eval_fss(d, model, opt.n_samples, thr_B, thr_A, win), dev_dataset,
                                 test_dataset, header)
        levels = opt.fss_thresholds if opt.fss_thresholds is not None else opt.fss_quantiles
        t, w = int(np.argmax(levels)), len(win) // 2     # the highest threshold, the median listed window
        print("DEV_FSS_B: %.4f, TEST_FSS_B: %.4f, TEST_FSS_PROB_B: %.4f, TEST_FSS_MEAN_B: %.4f, TEST_FSS_A: %.4f, "
              "TEST_USEFUL_SCALE_B: %.4f"
              % (_chan_mean(dev['fss_members_B'][:, t, w]), _chan_mean(test['fss_members_B'][:, t, w]),
                 _chan_mean(test['fss_ens_prob_B'][:, t, w]), _chan_mean(test['fss_ens_mean_B'][:, t, w]),
                 _chan_mean(test['fss_fake_A'][:, t, w]), float(test['useful_scale_members_B'][:, t].mean())))
    elif opt.metric == 'translate':
        plan = ops.window_plan(devA.shape[2], devA.shape[3], grid_size, opt.overlap)
        header = dict(n_samples=np.int64(opt.n_samples), window=np.int64(grid_size), overlap=np.int64(opt.overlap),
                      origins_y=np.array(plan.oy[:plan.ny], dtype=np.int64), origins_x=np.array(plan.ox[:plan.nx], dtype=np.int64))
        # batches of at most 8 fields: a batch's canvases of every member stay on the device until they are read
        small = lambda a, b: AlignedIterator(a, b, batch_size=cap(len(a), 8))
        rmse = []

        def translated(dataset):          # the file holds the maps; the two scalars are only printed
            res = eval_translate(dataset, model, opt.n_samples, opt.overlap)
            rmse.append((res.pop('rmse_mean_B'), res.pop('rmse_A')))
            return res
        _eval_splits(opt, 'translate', translated, small(devA, devB), small(testA, testB), header, dtype=np.float32)
        print("DEV_RMSE_MEAN_B: %.4f, TEST_RMSE_MEAN_B: %.4f, TEST_RMSE_A: %.4f" % (rmse[0][0], rmse[1][0], rmse[1][1]))
    elif opt.metric == 'field_spectrum':
        header = dict(n_samples=np.int64(opt.n_samples), window=np.int64(grid_size), overlap=np.int64(opt.overlap),
                      height=np.int64(devA.shape[2]), width=np.int64(devA.shape[3]))
        small = lambda a, b: AlignedIterator(a, b, batch_size=cap(len(a), 8))     # as translate: whole canvases of every member
        dev, test = _eval_splits(opt, 'field_spectrum', lambda d: eval_field_spectrum(d, model, opt.n_samples, opt.overlap),
                                 small(devA, devB), small(testA, testB), header)
        print("DEV_LSD_B: %.4f, TEST_LSD_B: %.4f, DEV_LSD_A: %.4f, TEST_LSD_A: %.4f, DEV_K_EFF_B: %.4f, TEST_K_EFF_B: %.4f"
              % (dev['lsd_B'], test['lsd_B'], dev['lsd_A'], test['lsd_A'], dev['k_eff_members_B'].mean(),
                 test['k_eff_members_B'].mean()))
    elif opt.metric == 'ssim':
        dev, test = _eval_splits(opt, 'ssim', lambda d: eval_ssim(d, model, opt.n_samples), dev_dataset, test_dataset,
                                 dict(n_samples=np.int64(opt.n_samples)), dtype=np.float64)
        print("DEV_SSIM_B: %.4f, TEST_SSIM_B: %.4f, TEST_CS_B: %.4f, TEST_SSIM_MEAN_B: %.4f, TEST_CS_MEAN_B: %.4f, "
              "TEST_SSIM_A: %.4f, TEST_CS_A: %.4f"
              % (dev['ssim_members_B'].mean(), test['ssim_members_B'].mean(), test['cs_members_B'].mean(),
                 test['ssim_ens_mean_B'].mean(), test['cs_ens_mean_B'].mean(), test['ssim_fake_A'].mean(),
                 test['cs_fake_A'].mean()))
    elif opt.metric == 'marginal':
        edges_B = marginal_edges(trainB, opt.marg_bins)            # once: dev and test share the climatology
        edges_A = marginal_edges(trainA, opt.marg_bins)
        levels = tuple(opt.marg_levels)
        header = dict(n_samples=np.int64(opt.n_samples), levels=np.array(levels, dtype=np.float64), edges_B=edges_B, edges_A=edges_A)
        dev, test = _eval_splits(opt, 'marginal', lambda d: eval_marginal(d, model, opt.n_samples, levels, edges_B, edges_A),
                                 dev_dataset, test_dataset, header)
        print("DEV_W1_B: %.4f, TEST_W1_B: %.4f, TEST_W1_MEAN_B: %.4f, TEST_W1_A: %.4f, TEST_KS_B: %.4f, TEST_KS_MEAN_B: %.4f, "
              "TEST_KS_A: %.4f"
              % (dev['w1_members_B'].mean(), test['w1_members_B'].mean(), test['w1_ens_mean_B'].mean(), test['w1_fake_A'].mean(),
                 test['ks_members_B'].mean(), test['ks_ens_mean_B'].mean(), test['ks_fake_A'].mean()))
    elif opt.metric == 'minkowski':
        thr_B = marginal_edges(trainB, opt.mink_bins)              # once: dev and test share the climatology
        thr_A = marginal_edges(trainA, opt.mink_bins)
        header = dict(n_samples=np.int64(opt.n_samples), bins=np.int64(opt.mink_bins), thresholds_B=thr_B, thresholds_A=thr_A)
        dev, test = _eval_splits(opt, 'minkowski', lambda d: eval_minkowski(d, model, opt.n_samples, thr_B, thr_A),
                                 dev_dataset, test_dataset, header)
        for name, res in (('DEV', dev), ('TEST', test)):
            print("%s_MINK_B: %s, %s_MINK_MEAN_B: %s, %s_MINK_A: %s (area, perimeter, euler4, euler8)"
                  % tuple(v for k in ('members_B', 'ens_mean_B', 'fake_A')
                          for v in (name, " ".join("%.6f" % _chan_mean(res['dist_%s_%s' % (f, k)]) for f in ops.MINK_FUNCTIONALS))))
    else:
        raise NotImplementedError('wrong metric!')
    return opt


if __name__ == "__main__":
    test_model()
