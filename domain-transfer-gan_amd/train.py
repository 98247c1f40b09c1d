#!/usr/bin/env python3
"""Training driver — Py3 counterpart of /root/reference/augmented_cyclegan/train.py:96-313 (Python 2 there).
Same flags (options.py), same `results.txt` line format (train.py:39-45), same artefacts: opt.txt / opt.pkl,
nets.txt, results.json, history_mse_A.npy / history_ubo_B.npy, best_mse_A.txt / best_bpp_B.txt, checkpoints
`latest` / `best_A` / `best_B`, PNG grids under vis_*/ (written by a small built-in PNG encoder: torchvision is not
required).  Additions: a working --continue_train, --synthetic data, one-process-per-GPU data parallelism
(`python -m torch.distributed.run --nproc-per-node N -m ...train` shards every batch by rank), --native_res (fields at
their stored resolution, a fresh random --grid_size window per sample and step)."""
import contextlib
import itertools
import json
import os
import random
import struct
import sys
import time
import zlib
from shutil import copyfile

import numpy as np
import torch

from . import dist as D, losses, ops
from .dataloader import AlignedIterator, DevicePrefetcher, UnalignedIterator, load_numpy_data, synthetic_data, window_tables
from .evaluate import eval_mse_A, eval_ubo_B, one_to_three_channels
from .model import AugmentedCycleGAN, DeferredStep, StochCycleGAN
from .options import TrainOptions, create_sub_dirs


def save_results(expr_dir, results_dict):
    with open(os.path.join(expr_dir, 'results.json'), 'w') as f:
        json.dump(results_dict, f, indent=4)


def print_log(out_f, message):
    if out_f is not None:
        out_f.write(message + "\n")
        out_f.flush()
        print(message)


def format_log(epoch, i, errors, t, prefix=True):
    """train.py:39-45"""
    message = '(epoch: %d, iters: %d, time: %.3f) ' % (epoch, i, t)
    if not prefix:
        message = ' ' * len(message)
    for k, v in errors.items():
        message += '%s: %.3f ' % (k, v)
    return message


def write_png(path, img_u8):
    """img_u8: (H, W, 3) uint8 -> minimal PNG (zlib + CRC chunks)"""
    h, w, _ = img_u8.shape
    raw = b''.join(b'\x00' + img_u8[y].tobytes() for y in range(h))

    def chunk(tag, data):
        c = struct.pack('>I', len(data)) + tag + data
        return c + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) +
                chunk(b'IDAT', zlib.compress(raw, 6)) + chunk(b'IEND', b''))


def save_image_grid(t, path, nrow, pad=2):
    """(N,3,H,W) in [-1,1] -> PNG grid with `nrow` images per row (vutils.save_image(normalize=True, range=(-1,1)))"""
    t = ((t.detach().float().cpu().clamp(-1, 1) + 1) * 127.5).round().byte().numpy()
    n, c, h, w = t.shape
    rows = (n + nrow - 1) // nrow
    grid = np.zeros((rows * (h + pad) + pad, nrow * (w + pad) + pad, 3), np.uint8)
    for i in range(n):
        r, q = divmod(i, nrow)
        grid[pad + r * (h + pad): pad + r * (h + pad) + h, pad + q * (w + pad): pad + q * (w + pad) + w] = t[i, :3].transpose(1, 2, 0)
    write_png(path, grid)


def visualize_cycle(opt, real_A, visuals, eidx, uidx, train):
    """train.py:47-59"""
    size = real_A.size()
    images = [one_to_three_channels(img.cpu()).unsqueeze(1) for img in visuals.values()]
    vis = torch.cat(images, dim=1).view(size[0] * len(images), 3, size[2], size[3])
    save_path = os.path.join(opt.train_vis_cycle if train else opt.vis_cycle, 'cycle_%02d_%04d.png' % (eidx, uidx))
    save_image_grid(vis, save_path, nrow=len(images))
    copyfile(save_path, os.path.join(opt.vis_latest, 'cycle.png'))


def visualize_multi(opt, real_A, model, eidx, uidx):
    """train.py:61-74"""
    size = real_A.size()
    z = real_A.new_empty((opt.num_multi, opt.nlatent, 1, 1)).normal_(0, 1).repeat(size[0], 1, 1, 1)
    with torch.no_grad():
        multi = model.generate_multi(real_A.detach(), z)
    multi = one_to_three_channels(multi.cpu()).view(size[0], opt.num_multi, 3, size[2], size[3])
    vis = torch.cat([one_to_three_channels(real_A.cpu()).unsqueeze(1), multi], dim=1).view(size[0] * (opt.num_multi + 1), 3, size[2], size[3])
    save_path = os.path.join(opt.vis_multi, 'multi_%02d_%04d.png' % (eidx, uidx))
    save_image_grid(vis, save_path, nrow=opt.num_multi + 1)
    copyfile(save_path, os.path.join(opt.vis_latest, 'multi.png'))


def _cuda(t, on):
    return t.cuda() if on else t


# --defer_scalars: at most this many replayed steps are in flight when the next one is enqueued
RUN_AHEAD = 2


class PinnedUploads(object):
    """Host -> device uploads that do not make the host wait for the compute stream (a pageable .cuda() copy does): each
    tensor is staged in one of a small ring of pinned buffers per (name, shape) and sent with non_blocking=True.  A buffer
    is overwritten only after the event of the copy that last read it has completed; with RUN_AHEAD steps in flight, three
    buffers per name never wait on a step still running."""
    SLOTS = 3

    def __init__(self, device):
        self.device, self.rings = device, {}

    def __call__(self, name, t):
        ring = self.rings.get((name, tuple(t.shape)))
        if ring is None:
            ring = self.rings[(name, tuple(t.shape))] = dict(
                bufs=[torch.empty(t.shape, dtype=t.dtype).pin_memory() for _ in range(self.SLOTS)],
                events=[None] * self.SLOTS, next=0)
        i = ring['next']
        ring['next'] = (i + 1) % self.SLOTS
        if ring['events'][i] is not None:
            ring['events'][i].synchronize()     # that buffer's previous copy has left host memory
        buf = ring['bufs'][i]
        buf.copy_(t)
        out = buf.to(self.device, non_blocking=True)
        ev = ring['events'][i] = torch.cuda.Event()
        ev.record()
        return out


class Trainer(object):
    """One training run: data -> model -> epochs of train_instance (+ optional paired step) -> per-epoch checkpoint,
    evaluation, best-model tracking and LR decay.  Rank 0 owns all files; every rank trains on its shard of each batch."""

    BEST = ('best_dev_mse_A', 'best_test_mse_A', 'best_dev_bpp_B', 'best_test_bpp_B')

    def __init__(self, argv=None):
        self.opt = opt = TrainOptions().parse(sub_dirs=['vis_multi', 'vis_cycle', 'vis_latest', 'train_vis_cycle'], argv=argv)
        self.rank, self.ws = D.init_from_env()
        self.gpu = len(opt.gpu_ids) > 0
        self.log_f = open("%s/results.txt" % opt.expr_dir, 'a' if opt.continue_train else 'w') if self.rank == 0 else None
        ops.set_precision(opt.precision)
        if opt.seed is not None:                                                         # train.py:102-108
            print("using random seed:", opt.seed)
            random.seed(opt.seed); np.random.seed(opt.seed); torch.manual_seed(opt.seed)
            if self.gpu:
                torch.cuda.manual_seed_all(opt.seed)
        self._data()
        self._model()
        self.total_steps = 0
        self.results = {k: sys.float_info.max for k in self.BEST}
        self.history_mse_A, self.history_ubo_B = [], []
        if self.rank == 0:
            save_results(opt.expr_dir, self.results)
        create_sub_dirs(opt, ['vis_pred_B'])

    def log(self, msg):
        print_log(self.log_f, msg)

    # ---------------------------------------------------------------- setup
    def _data(self):
        o = self.opt
        if o.synthetic:
            arrays = synthetic_data(o.synthetic, o.input_nc, o.output_nc, o.grid_size, o.seed or 0)
        else:
            arrays = load_numpy_data(o.dataroot, grid_size=o.grid_size, native_res=bool(getattr(o, "native_res", False)))
        trainA, trainB, devA, devB, testA, testB = arrays
        self.train_it = UnalignedIterator(trainA, trainB, batch_size=o.batchSize)
        self.test_it = AlignedIterator(testA, testB, batch_size=100)
        self.dev_it = AlignedIterator(devA, devB, batch_size=100)
        self.dev_cycle = itertools.cycle(AlignedIterator(devA, devB, batch_size=25))
        for label, it in (('training', self.train_it), ('test', self.test_it), ('dev', self.dev_it)):
            self.log('#%s images = %d' % (label, len(it)))
        self.sup_it = None
        if o.supervised:
            n_sup = int(len(trainA) * o.sup_frac)
            self.sup_it = itertools.cycle(AlignedIterator(trainA[:n_sup], trainB[:n_sup], batch_size=o.batchSize))
            self.log('#supervised images = %d' % n_sup)
        if losses.BY_STEM["fss"].on(o):
            self._fss_loss_thresholds(trainA, trainB)

    def _fss_loss_thresholds(self, trainA, trainB):
        """--lambda_fss_A / --lambda_fss_B: the event thresholds of the loss, once, from the real training fields - the
        climatology --metric fss uses (eval_metrics.fss_thresholds) - as (C, T) nested lists on the options, so that the
        model finds them and opt.pkl carries them to whoever reloads the run"""
        from .eval_metrics import fss_thresholds
        o = self.opt
        for name, train in (("A", trainA), ("B", trainB)):
            thr = fss_thresholds(train, o.fss_loss_quantiles, o.fss_loss_thresholds)
            setattr(o, "fss_loss_thr_" + name, [[float(v) for v in row] for row in thr])
            self.log("fss loss thresholds %s (%s): %s" % (name, "explicit" if o.fss_loss_thresholds is not None else
                                                          "quantiles %s" % (tuple(o.fss_loss_quantiles),),
                                                          "; ".join("channel %d: %s" % (c, ", ".join("%.6g" % v for v in row))
                                                                    for c, row in enumerate(thr))))
        if self.rank == 0:                                         # the options on disk were written before the data was read
            import pickle
            path = os.path.join(o.expr_dir, "opt.pkl")
            with open(path, "rb") as f:
                saved = pickle.load(f)
            saved.update(fss_loss_thr_A=o.fss_loss_thr_A, fss_loss_thr_B=o.fss_loss_thr_B)
            with open(path, "wb") as f:
                pickle.dump(saved, f)

    def _model(self):
        o = self.opt
        if o.model == 'aug_cycle_gan':
            self.model = AugmentedCycleGAN(o)
            create_sub_dirs(o, ['vis_inf'])
        elif o.model in ('stoch_cycle_gan', 'cycle_gan'):
            self.model = StochCycleGAN(o, ignore_noise=(o.model == 'cycle_gan'))
        else:
            raise NotImplementedError('Specified model is not implemented.')
        self.log("model [%s] was created (conv arithmetic: %s, %d rank%s)"
                 % (self.model.__class__.__name__, ops.get_precision(), self.ws, "" if self.ws == 1 else "s"))
        self.defer = bool(getattr(o, "defer_scalars", False))
        if getattr(o, "step_graph", False):           # both steps (unsupervised and paired) replay from graphs; ignored while
            self.model.enable_step_graph(defer_scalars=self.defer)   # the data-parallel exchange is on (model.train_instance)
        self.upload = PinnedUploads(torch.device("cuda")) if self.defer and self.gpu else None
        # --ema_decay with --ema_eval 1: the evaluation and the dev-set pictures run on the averaged weights
        self.ema_eval = bool(getattr(o, "ema_decay", 0.0) > 0 and getattr(o, "ema_eval", 1))
        if o.continue_train:
            chk = os.path.join(o.expr_dir, o.which_epoch)
            self.model.load(chk)
            self.log("continue_train: loaded %s" % chk)

    # ---------------------------------------------------------------- one epoch
    def _shard(self, t):
        if self.ws == 1:
            return t
        n = t.size(0) // self.ws
        return t[self.rank * n:(self.rank + 1) * n]

    def _scored(self):
        """the weights the evaluation and the dev-set pictures see: the model's averaged ones (model.ema_weights) under
        --ema_decay with --ema_eval 1, else the live ones"""
        return self.model.ema_weights() if self.ema_eval else contextlib.nullcontext()

    def _visualize(self, real_A, visuals, epoch, it):
        o, m = self.opt, self.model
        visualize_cycle(o, real_A, visuals, epoch, it, train=True)
        batch = next(self.dev_cycle)
        dA, dB = _cuda(batch['A'], self.gpu), _cuda(batch['B'], self.gpu)
        dz = dA.new_empty((dA.size(0), o.nlatent, 1, 1)).normal_(0, 1)
        with self._scored():
            with torch.no_grad():
                visualize_cycle(o, dA, m.generate_cycle(dA, dB, dz), epoch, it, train=False)
            visualize_multi(o, dA, m, epoch, it)

    def _train_batches(self):
        """this rank's shard of every training batch; on the GPU the next batch is uploaded through pinned memory on a
        side stream while the current step computes (dataloader.DevicePrefetcher)"""
        class Sharded(object):          # host-side shard BEFORE the upload: a rank moves only its own rows
            def __init__(s, it):
                s.it = it

            def __len__(s):
                return len(s.it)

            def __iter__(s):
                iter(s.it)
                return s

            def __next__(s):
                d = next(s.it)
                full = d['A'].size(0)
                return {'A': self._shard(d['A']), 'B': self._shard(d['B']), 'n': (full, d['B'].size(0))}
        src = Sharded(self.train_it)
        return DevicePrefetcher(src) if self.gpu else src

    def _to_device(self, name, t):
        if self.upload is not None:
            return self.upload(name, t)
        return _cuda(t, self.gpu)

    def _windows(self, name, real_A, real_B, n_full, paired=False):
        """--native_res: this rank's fields (n, C, H, W) of a batch of n_full -> their random grid_size windows, NCHW as the
        step takes them.  The tables are drawn on the host for the full batch (dataloader.window_tables; np.random, so
        --seed reproduces them), sharded like prior_z_B and uploaded like it; paired: one table for both sides.  Two
        launches per side (ops.window_gather, ops.ToNCHW), before the step and outside its captured graph."""
        o = self.opt
        tabs = window_tables(n_full, real_A.shape[2:], real_B.shape[2:], o.grid_size, flip=bool(o.window_flip), paired=paired)
        out = []
        for side, x, tab in zip("AB", (real_A, real_B), tabs):
            tab = self._shard(torch.from_numpy(tab)).clone()
            tab[:, 0] -= tab[0, 0].clone()                     # src counts inside this rank's shard
            y = ops.window_gather(x, tab, o.grid_size, upload=lambda t, k="%s_%s" % (name, side): self._to_device(k, t))
            out.append(ops.ToNCHW.apply(y, x.size(1)))
        return out

    def train_epoch(self, epoch):
        """one pass over the training batches.  Under --defer_scalars a replayed step returns a model.DeferredStep: its
        numbers are read (.result()) only on a step that logs or visualises, before the next step is enqueued (its visuals
        are the graph's static buffers), and at most RUN_AHEAD steps are in flight."""
        o, m = self.opt, self.model
        native = bool(getattr(o, "native_res", False))        # options saved before the flag existed: off
        seen = 0
        in_flight = []
        for data in self._train_batches():
            real_A, real_B = data['A'], data['B']
            nA, nB = data['n']
            if nA != nB:
                continue
            prior_z_B = torch.empty((nA, o.nlatent, 1, 1)).normal_(0, 1)                 # on the host, train.py:193
            self.total_steps += o.batchSize
            seen += o.batchSize
            if len(in_flight) >= RUN_AHEAD:
                in_flight.pop(0).wait()
            prior_z_B = self._to_device('prior_z_B', self._shard(prior_z_B))
            if native:
                real_A, real_B = self._windows('win', real_A, real_B, nA)
            out = m.train_instance(real_A, real_B, prior_z_B)
            sup_losses = None
            if self.sup_it is not None:
                sd = next(self.sup_it)
                sA, sB = self._to_device('sup_A', self._shard(sd['A'])), self._to_device('sup_B', self._shard(sd['B']))
                if native:
                    sA, sB = self._windows('sup_win', sA, sB, sd['A'].size(0), paired=True)
                sup_losses = m.supervised_train_instance(sA, sB, prior_z_B[:sA.size(0)])
            last = sup_losses if sup_losses is not None else out
            if isinstance(last, DeferredStep):     # completes after everything this iteration enqueued
                in_flight.append(last)
            display = self.total_steps % o.display_freq == 0 and self.rank == 0
            if display or self.total_steps % o.print_freq == 0:
                out = out.result() if isinstance(out, DeferredStep) else out
                sup_losses = sup_losses.result() if isinstance(sup_losses, DeferredStep) else sup_losses
            if display:
                self._visualize(real_A, out[1], epoch, seen // o.batchSize)
            if self.total_steps % o.print_freq == 0:
                t = (time.time() - self.tick) / o.batchSize                            # seconds per image, train.py:243
                self.log(format_log(epoch, seen, out[0], t))
                if sup_losses is not None:
                    self.log(format_log(epoch, seen, sup_losses, t, prefix=False))
                if o.monitor_gnorm:
                    self.log(format_log(epoch, seen, out[2], t, prefix=False) + "\n")
                self.tick = time.time()

    # ---------------------------------------------------------------- per-epoch evaluation (rank 0)
    def _track_best(self, epoch, line, dev, test, dev_key, test_key, chk, fname, banner):
        o = self.opt
        lines = [line]
        if dev < self.results[dev_key]:
            with open(os.path.join(o.expr_dir, fname), 'w') as f:
                f.write(line + '\n')
            self.results[dev_key], self.results[test_key] = dev, test
            self.model.save(chk)
            save_results(o.expr_dir, self.results)
            lines.append(banner)
        self.log("\n".join(["-" * 60] + lines + ["-" * 60]))

    def evaluate(self, epoch):
        o, m = self.opt, self.model
        if epoch % o.eval_A_freq == 0:
            t0 = time.time()
            dev, test = eval_mse_A(self.dev_it, m, self.gpu), eval_mse_A(self.test_it, m, self.gpu)
            self.history_mse_A.append((dev, test))
            np.save("%s/history_mse_A" % o.expr_dir, self.history_mse_A)
            line = "[%d] DEV_MSE_A: %.4f, TEST_MSE_A: %.4f, TIME: %.4f" % (epoch, dev, test, time.time() - t0)
            self._track_best(epoch, line, dev, test, 'best_dev_mse_A', 'best_test_mse_A', 'best_A', 'best_mse_A.txt',
                             "*** BEST DEV A ***")
        if epoch % o.eval_B_freq == 0:
            t0 = time.time()
            steps = 1 if o.model == 'cycle_gan' else o.eval_steps                      # train.py:281-285
            d_ubo, d_bpp, d_kld = eval_ubo_B(self.dev_it, m, steps, self.gpu)
            t_ubo, t_bpp, t_kld = eval_ubo_B(self.test_it, m, steps, self.gpu)
            self.history_ubo_B.append((d_ubo, d_bpp, d_kld, t_ubo, t_bpp, t_kld))
            np.save("%s/history_ubo_B" % o.expr_dir, self.history_ubo_B)
            line = "[%d] DEV_BPP_B: %.4f, TEST_BPP_B: %.4f, TIME: %.4f" % (epoch, d_bpp, t_bpp, time.time() - t0)
            self._track_best(epoch, line, d_bpp, t_bpp, 'best_dev_bpp_B', 'best_test_bpp_B', 'best_B', 'best_bpp_B.txt',
                             "*** BEST BPP B ***")

    def run(self):
        o = self.opt
        self.tick = time.time()
        last = o.niter + o.niter_decay
        for epoch in range(o.epoch_count, last + 1):
            t0 = time.time()
            self.train_epoch(epoch)
            if self.rank == 0:
                if epoch % o.save_epoch_freq == 0:
                    self.log('saving the model at the end of epoch %d, iters %d' % (epoch, self.total_steps))
                    self.model.save('latest')
                if self.ema_eval:
                    self.log("[%d] evaluating the averaged weights (ema_decay %g); the checkpoints hold the live weights "
                             "under the usual keys and the averaged ones under ema_<net>" % (epoch, o.ema_decay))
                with self._scored():
                    self.evaluate(epoch)
            self.log('End of epoch %d / %d \t Time Taken: %d sec' % (epoch, last, time.time() - t0))
            if epoch > o.niter:
                self.model.update_learning_rate()
        if self.log_f is not None:
            self.log_f.close()
        return self.model


def train_model(argv=None):
    """entry point with the reference's name (train.py:96)"""
    return Trainer(argv).run()


if __name__ == "__main__":
    train_model()
