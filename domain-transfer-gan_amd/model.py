"""Training-step orchestration — the API surface of /root/reference/augmented_cyclegan/model.py
(StochCycleGAN, AugmentedCycleGAN with train_instance / supervised_train_instance / generate_* /
predict_* / save / load / update_learning_rate / eval / train, plus the loss helpers), running on
the HIP kernels of libacgan_hip.so.

What differs from the reference, by design:
  * train_instance returns python floats exactly like the reference, but gathers all 13 losses and
    the monitors with ONE device->host copy per step instead of 19 syncs;
  * per-network clip_grad_norm + Adam are one fused kernel per network on flat buffers, the clip
    coefficient is read on the device;
  * in the G phase the discriminators' (discarded) weight gradients are not computed;
  * multi-GPU = one process per GPU, gradients averaged by RCCL all-reduce before clipping (dist.py).
Aliases for the north-star names: AugmentedCycleGAN_Model, .optimize_parameters(), .set_input().
"""
import contextlib
import functools  # noqa: F401
import math
import os
from collections import OrderedDict

import numpy as np  # noqa: F401
import torch

from . import dist as acg_dist
from . import losses, networks, ops
from .losses import hashable as _hashable
from .modules import _starts_with_conv, as_latent, mark_dirty, packed_of, repack
from .ops import cpad


# ------------------------------------------------------------------------------------------------
# loss helpers (model.py:15-72) — tensor functions, autograd-capable, device-agnostic
# ------------------------------------------------------------------------------------------------
def gauss_reparametrize(mu, logvar, n_sample=1):
    """model.py:15-22"""
    std = logvar.mul(0.5).exp()
    size = std.size()
    eps = std.new_empty((size[0], n_sample, size[1])).normal_()
    z = eps.mul(std[:, None, :]).add(mu[:, None, :])
    z = torch.clamp(z, -4., 4.)
    return z.view(z.size(0) * z.size(1), z.size(2), 1, 1)


def log_prob_laplace(z, mu, log_var):
    """model.py:24-28"""
    sd = torch.exp(0.5 * log_var)
    res = - 0.5 * log_var - (torch.abs(z - mu) / sd)
    return res + (-math.log(2))


def log_prob_gaussian(z, mu, log_var):
    """model.py:31-34"""
    res = - 0.5 * log_var - ((z - mu) ** 2.0 / (2.0 * torch.exp(log_var)))
    return res - 0.5 * math.log(2 * math.pi)


def kld_std_guss(mu, log_var):
    """model.py:45-53"""
    return -0.5 * torch.sum(log_var + 1. - mu ** 2 - torch.exp(log_var), dim=1)


def criterion_GAN(pred, target_is_real, use_sigmoid=True):
    """model.py:56-72.  `pred` is an NCHW / (N,1) tensor (public API form).  The use_sigmoid branch is the reference's,
    which cannot run (below); --no_lsgan models use criterion_GAN_bce instead."""
    if use_sigmoid:
        raise NotImplementedError("use_sigmoid: the reference's BCE branch builds a Long target and fails on modern torch "
                                  "(model.py:59-63); use criterion_GAN_bce (what --no_lsgan models train with)")
    t = 1.0 if target_is_real else 0.0
    p = pred.reshape(-1, 1).contiguous()
    return ops.MseConst.apply(_pad_cols(p, 4), 1, t)


def criterion_GAN_bce(pred, target_is_real):
    """The vanilla-GAN objective of --no_lsgan (model.py:56-63 with its one bug fixed: the target is FLOAT, the reference's
    Long target is rejected by F.binary_cross_entropy).  `pred` = sigmoid(head(x)), what a use_sigmoid discriminator
    returns (NCHW / (N,1)); the loss is F.binary_cross_entropy(pred, full_like(pred, t)), t = 1. or 0.:
    mean(-(t max(log p, -100) + (1 - t) max(log(1 - p), -100))), gradient g (p - t) / max(p (1 - p), 1e-12) / count.
    The sigmoid stays a step of its own (fused into the head's epilogue, backward dy y (1 - y)), as in the reference
    composite: no BCE-with-logits rewrite, whose values differ at saturation."""
    t = 1.0 if target_is_real else 0.0
    p = pred.reshape(-1, 1).contiguous()
    return ops.BceConst.apply(_pad_cols(p, 4), 1, t)


def _pad_cols(p, Cp):
    out = p.new_zeros((p.shape[0], Cp))
    out[:, :p.shape[1]] = p
    return out


def _gan_loss(pred_c16, target_is_real, bce=False):
    """The GAN loss on an internal C16 prediction map (1 valid channel): LSGAN, or with bce (--no_lsgan) the binary
    cross-entropy of criterion_GAN_bce on the sigmoid map."""
    return (ops.BceConst if bce else ops.MseConst).apply(pred_c16, 1, 1.0 if target_is_real else 0.0)


# ------------------------------------------------------------------------------------------------
# flat parameter storage + fused clip/Adam
# ------------------------------------------------------------------------------------------------
class FlatNet(object):
    """All parameters (and their .grad) of one network as views into single flat fp32 buffers —
    what the fused l2-norm / clip / Adam kernels and the RCCL all-reduce operate on."""

    def __init__(self, net):
        self.net = net
        self.params = [p for p in net.parameters()]
        dev = self.params[0].device
        offs, n = [], 0
        for p in self.params:
            offs.append(n)
            n += (p.numel() + 3) // 4 * 4
        self.n = n
        self.p = torch.zeros(n, device=dev, dtype=torch.float32)
        # the gradient buffer carries dist.SCALAR_TAIL extra floats: the all-reduce of the buffer also averages the
        # step's reported scalars written there (no separate collective, no host sync)
        self.g = torch.zeros(n + acg_dist.SCALAR_TAIL, device=dev, dtype=torch.float32)
        self.gv, self.gtail = self.g[:n], self.g[n:]
        self.m = torch.zeros(n, device=dev, dtype=torch.float32)
        self.v = torch.zeros(n, device=dev, dtype=torch.float32)
        self.offs = offs
        with torch.no_grad():
            for p, o in zip(self.params, offs):
                self.p[o:o + p.numel()].copy_(p.reshape(-1))
                p.data = self.p[o:o + p.numel()].view(p.shape)
                p.grad = self.g[o:o + p.numel()].view(p.shape)
                p._acg_direct_grad = True    # ops: weight-gradient kernels add straight into this view
        self.sumsq = torch.zeros((), device=dev, dtype=torch.float32)
        mark_dirty(net)
        self._exchange = None
        if acg_dist.exchange_on():
            acg_dist.hook_params(self)

    def enable_ema(self):
        """allocate `ema`: the exponential moving average of `p` (n floats, starts as a copy), kept by FusedAdam behind every
        step.  A FlatNet without it has no such attribute."""
        self.ema = self.p.clone()

    def check(self):
        p0 = self.params[0]
        if p0.data_ptr() != self.p.data_ptr() or p0.grad is None or p0.grad.data_ptr() != self.g.data_ptr():
            raise RuntimeError("network parameters were re-allocated after the model was built (e.g. .cuda()/.to()); "
                               "build the model on its final device")

    def zero_grad(self):
        self.g.zero_()

    def set_requires_grad(self, flag):
        for p in self.params:
            p.requires_grad_(flag)


class FusedAdam(object):
    """torch.optim.Adam(lr, betas=(beta1, 0.999)) over one or more FlatNets, with the reference's
    per-network clip_grad_norm folded in (model.py:379-389, 447-452, 510-515).
    Exposes `param_groups` (update_learning_rate mutates 'lr') and torch-compatible state dicts."""

    def __init__(self, flats, lr, betas, eps=1e-8):
        self.flats = list(flats)
        self.param_groups = [dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False)]
        self.t = 0
        self.t_dev = None      # int32 device copy of t, read by the kernels of a captured step graph (StepGraph)
        self.dev_step = False  # True only while StepGraph captures: the recorded launches take the step from t_dev
        self.ema_decay = 0.0   # the decay of the flats' averages (those that have one: FlatNet.enable_ema), set by the model

    def zero_grad(self):
        for f in self.flats:
            f.zero_grad()

    def clip_and_step(self, max_norm):
        """per network: sumsq -> (device) clip coefficient -> Adam.  Returns the sumsq scalars."""
        g = self.param_groups[0]
        self.t += 1
        ops.clip_adam_multi([(f.p, f.gv, f.m, f.v, f.sumsq) for f in self.flats], max_norm, g['lr'], g['betas'][0],
                            g['betas'][1], g['eps'], self.t, self.t_dev if self.dev_step else None)
        avg = [(f.p, f.ema) for f in self.flats if hasattr(f, "ema")]
        if avg:                # the averaged weights follow the step just taken: one launch, the step number as Adam's
            ops.ema_multi(avg, self.ema_decay, self.t, self.t_dev if self.dev_step else None)
        for f in self.flats:   # the packed copies follow the parameters: one launch per network (modules.repack)
            repack(f.net)
        return [f.sumsq for f in self.flats]

    def state_dict(self):
        state, idx = {}, 0
        for f in self.flats:
            for p, o in zip(f.params, f.offs):
                n = p.numel()
                state[idx] = dict(step=torch.tensor(float(self.t)), exp_avg=f.m[o:o + n].view(p.shape).clone(),
                                  exp_avg_sq=f.v[o:o + n].view(p.shape).clone())
                idx += 1
        pg = dict(self.param_groups[0])
        pg['params'] = list(range(idx))
        return dict(state=state, param_groups=[pg])

    def load_state_dict(self, sd):
        idx = 0
        for f in self.flats:
            for p, o in zip(f.params, f.offs):
                st = sd['state'].get(idx)
                if st is not None:
                    n = p.numel()
                    f.m[o:o + n].copy_(st['exp_avg'].reshape(-1))
                    f.v[o:o + n].copy_(st['exp_avg_sq'].reshape(-1))
                    self.t = int(float(st['step']))
                idx += 1
        self.param_groups[0]['lr'] = sd['param_groups'][0]['lr']


class _PendingVals(object):
    """the step's scalars still on the device (graph capture): names, the stacked tensor and the closure that turns the
    host-side values into what train_instance returns"""

    def __init__(self, names, dev):
        self.names, self.dev, self.finish = names, dev, None

    def resolve(self):
        return self.finish(OrderedDict(zip(self.names, self.dev.tolist())))


class DeferredStep(object):
    """What `train_instance` returns under `enable_step_graph(defer_scalars=True)`: the step's reported scalars are on their way
    to pinned host memory (an asynchronous copy enqueued behind the replay); `result()` waits for that copy and builds the
    usual (losses, visuals[, gnorms]) — so the host can enqueue step k + 1 while step k runs and read step k's losses later
    (the reference's loop reads them every step, train.py:198-243; a loop that logs every n-th step need not wait every step).
    The tensors in `visuals` are the graph's static buffers: overwritten by the next step."""

    def __init__(self, pending, host, event):
        self._pending, self._host, self._event, self._out = pending, host, event, None

    def wait(self):
        """block the host until the step (and its scalars' copy) has completed on the device"""
        self._event.synchronize()

    def result(self):
        if self._out is None:
            self.wait()
            self._out = self._pending.finish(OrderedDict(zip(self._pending.names, self._host.tolist())))
        return self._out


class StepGraph(object):
    """train_instance captured into a HIP graph (torch.cuda.CUDAGraph drives hipStreamBeginCapture / hipGraphLaunch; the
    library's ctypes launches go to the capturing stream like torch's own kernels).  What a replay cannot take from the
    host is kept on the device: the inputs (static buffers copied into), the Adam step number (FusedAdam.t_dev, read by
    acg_clip_adam_multi) and the reported scalars (one .tolist() after the replay).  The learning rates are launch
    arguments: a change re-captures.  `step` names the model's step method: `_train_instance` (default) or
    `_supervised_train_instance` (the paired step, a second instance with its own warm-up, key, inputs and scratch).  Every
    instance checks the packed weights it was captured with before each of its replays."""
    WARMUP = 2

    def __init__(self, model, step="_train_instance"):
        self.model, self.graph, self.key, self.calls, self.ws, self.packed = model, None, None, 0, None, None
        self.step = step
        self.defer_scalars = False
        self.captures = 0      # completed captures (a re-capture after a learning-rate change counts again)
        self.stepped = None    # the optimisers whose Adam step the captured step takes (the paired step leaves D_A alone)

    def _key(self, a, b, z):
        m = self.model
        lrs = tuple(opt.param_groups[0]['lr'] for opt in m._optimizers().values())
        # everything a captured launch bakes in as an argument: shapes, learning rates, train/eval mode, the kernel
        # configuration (precision / implementation switch) and the scalar options of the step: those of no loss family
        # here, every family's own from its record
        own = ("max_gnorm", "lambda_A", "lambda_B", "lambda_z_B", "lambda_sup_A", "lambda_sup_B", "stoch_enc", "z_gan", "beta1",
               "ema_decay")
        baked = tuple(_hashable(getattr(m.opt, k, None)) for k in own + tuple(losses.key_options()))
        return (tuple(a.shape), tuple(b.shape), tuple(z.shape), lrs, m.netG_A_B.training, ops.CONFIG_EPOCH, baked)

    def _capture(self, key, real_A, real_B, prior_z_B):
        m = self.model
        opts = list(m._optimizers().values())
        inputs = [real_A.clone(), real_B.clone(), prior_z_B.clone()]
        for opt in opts:
            if opt.t_dev is None:
                opt.t_dev = torch.zeros(1, dtype=torch.int32, device=real_A.device)
        graph = torch.cuda.CUDAGraph()
        # every derived tensor the step uses must be current at every replay.  The packed convolution weights are: each
        # optimiser step refreshes them IN PLACE (modules.repack) — eagerly and inside the graph alike — so the objects the
        # layers hold now are baked in as they are (round 6: rebuilding them inside the graph cost every replay 68 pack
        # launches), kept alive by this object and checked before every replay.  The other derived forms (padded norm
        # vectors) are copies a kernel made once: those are rebuilt INSIDE the graph.
        for net in m._nets():
            mark_dirty(net, keep_packed=True)
        # ... and so must the scratch buffers: the captured kernels keep the workspace POINTERS, and ops.workspace() replaces
        # an eager buffer as soon as a later eager op (a larger evaluation batch) needs more.  The capture therefore starts
        # from an empty workspace table, so its buffers come from the graph's private pool, and this object keeps them alive;
        # the eager table is put back afterwards.
        eager_ws, ops._WS = ops._WS, {}
        t_before = [opt.t for opt in opts]
        m._capturing = True
        for opt in opts:
            opt.dev_step = True
        # Python's cyclic collector must not run inside the capture: what it finds may own device objects of an EARLIER graph
        # (another model's StepGraph in a reference cycle: its hipGraph and private pool), and destroying those while a stream is
        # capturing is an error raised in a destructor, i.e. an abort.  torch.cuda.graph() collects once before it starts.
        import gc
        gc_was_on = gc.isenabled()
        gc.collect()
        gc.disable()
        try:
            with torch.cuda.graph(graph), _in_train_step():
                pending = getattr(m, self.step)(*inputs)
            graph_ws = ops._WS
            stepped = [opt for opt, t in zip(opts, t_before) if opt.t != t]
        finally:
            if gc_was_on:
                gc.enable()
            ops._WS = eager_ws
            m._capturing = False
            for opt, t in zip(opts, t_before):     # the capture ran clip_and_step's host side without executing it
                opt.t = t
                opt.dev_step = False
        # only a capture that completed is kept: a failed one leaves no half-built graph behind for the next call to replay
        self.graph, self.key, self.inputs, self.pending, self.ws = graph, key, inputs, pending, graph_ws
        self.stepped = stepped
        self.packed = [packed_of(net) for net in m._nets()]     # (strong references: the graph holds their device pointers)
        self.captures += 1

    def __call__(self, real_A, real_B, prior_z_B):
        m = self.model
        key = self._key(real_A, real_B, prior_z_B)
        self.calls += 1
        if self.calls <= self.WARMUP:                 # lazily built state (packed weights, workspaces) settles eagerly
            with _in_train_step():
                return getattr(m, self.step)(real_A, real_B, prior_z_B)
        if self.graph is not None and key == self.key:
            # the layers must still hold the packed weights the graph was captured with (a checkpoint load, a precision switch or
            # mark_dirty() in between replaces them): otherwise capture again
            now = [packed_of(net) for net in m._nets()]
            if any(a is not b for pa, pb in zip(now, self.packed) for a, b in zip(pa, pb)):
                self.graph = None
        if self.graph is None or key != self.key:
            if self.graph is not None and self.defer_scalars:
                torch.cuda.current_stream().synchronize()   # earlier replays of the graph dropped here may still be running
            self.graph = self.key = None
            self._capture(key, real_A, real_B, prior_z_B)
        for dst, src in zip(self.inputs, (real_A, real_B, prior_z_B)):
            dst.copy_(src)
        for opt in self.stepped:
            opt.t_dev.fill_(opt.t)
        self.graph.replay()
        for opt in self.stepped:
            opt.t += 1
        deferred = None
        if self.defer_scalars:   # the scalars leave for pinned memory behind the replay; nobody waits here
            host = torch.empty(self.pending.dev.shape, dtype=self.pending.dev.dtype, pin_memory=True)
            host.copy_(self.pending.dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            deferred = DeferredStep(self.pending, host, ev)
        for net in m._nets():    # the replay updated the weights behind Python's caches (and repacked the convolutions' in place)
            mark_dirty(net, keep_packed=True)
        return deferred if deferred is not None else self.pending.resolve()


class _Base(object):
    def _gan_loss(self, pred_c16, target_is_real):
        """the model's criterionGAN on an internal prediction map: LSGAN, or BCE under --no_lsgan"""
        return _gan_loss(pred_c16, target_is_real, bool(self.opt.use_sigmoid))

    def _dev(self):
        return next(self.netG_A_B.parameters()).device

    def _optional_terms(self, loss, lams, fake_A, A, fake_B, B):
        """An optional loss family on the first-pass outputs against the real batches (`loss(fake, real, C, "nhwc")` on the
        internal NHWC tensors; unpaired: batch statistics): None when both weights are 0 (the default: no launch is issued),
        else (term_A, term_B, weighted sum for loss_G).  A term of weight 0 is a monitor without gradient.  `loss` may be a
        pair (loss of the A side, loss of the B side) where the sides differ in more than their operands."""
        lam_A, lam_B = lams
        if lam_A <= 0 and lam_B <= 0:
            return None
        loss_A, loss_B = loss if isinstance(loss, tuple) else (loss, loss)

        def term(loss, fake, real, C, lam):
            if lam > 0:
                return loss(fake, real, C, "nhwc")
            with torch.no_grad():
                return loss(fake.detach(), real, C, "nhwc")
        t_A = term(loss_A, fake_A, A, self.opt.input_nc, lam_A)
        t_B = term(loss_B, fake_B, B, self.opt.output_nc, lam_B)
        add = None
        for v, lam in ((t_A, lam_A), (t_B, lam_B)):
            if lam > 0:
                add = v * lam if add is None else add + v * lam
        return t_A, t_B, add

    def _nchw(self, x, C):
        return ops.ToNCHW.apply(x, C).detach()

    def _backward(self, loss, phase, order, tail=None):
        """loss.backward() with the gradient exchange of this optimiser phase overlapped (dist.PhaseExchange): `order` =
        the FlatNets in the order their gradients complete; tail = (carrier FlatNet, sum scalars, min/max monitors) rides
        behind the carrier's gradients.  Returns the exchange (wait(flat) before that network's clip) or None."""
        if not acg_dist.exchange_on():
            loss.backward()
            return None
        ex = self._exchanges.setdefault(phase, acg_dist.PhaseExchange(phase))
        if tail is not None:
            acg_dist.write_scalar_tail(tail[0].gtail, tail[1], tail[2] if len(tail) > 2 else None)
        ex.arm(order)
        try:
            with _in_train_step():
                loss.backward()
        finally:
            ex.flush()
        return ex

    @staticmethod
    def _wait(ex, *flats):
        if ex is not None:
            for f in flats:
                ex.wait(f)

    def _scalars(self, ex, carrier, names, sums, mins=(), maxs=(), local=()):
        """ONE device->host copy for every reported scalar.  `sums` are rank-averaged, `mins`/`maxs` reduced over ranks
        (both through the carrier's gradient tail when the exchange is on), `local` = values that are already identical
        on every rank (norms of the averaged gradients)."""
        sums = [t.detach().reshape(()).float() for t in sums]
        mm = [t.detach().reshape(()).float() for t in list(mins) + list(maxs)]
        if ex is not None:
            avg, per_rank = acg_dist.read_scalar_tail(carrier.gtail, len(sums), len(mm))
            sums = list(avg.unbind(0))
            if mm:
                mm = [per_rank[:, i].min() for i in range(len(mins))] + \
                     [per_rank[:, len(mins) + i].max() for i in range(len(maxs))]
        dev = torch.stack(sums + [t.detach().reshape(()).float() for t in local] + mm)
        if self._capturing:        # StepGraph: the copy to the host happens after the replay
            return _PendingVals(names, dev)
        return OrderedDict(zip(names, dev.tolist()))

    _capturing = False
    _step_graph = None
    _sup_step_graph = None

    def _report(self, vals, finish):
        """finish(vals) builds what the step returns from the host-side scalars; deferred while a graph is being captured"""
        if isinstance(vals, _PendingVals):
            vals.finish = finish
            return vals
        return finish(vals)

    def enable_step_graph(self, on=True, defer_scalars=False):
        """Run train_instance as ONE captured HIP graph per (shapes, learning rates): the whole step — about 3 000 kernel
        launches — is replayed by a single host call.  Worth it where the step is launch-bound (small images / batches:
        64 x 64 x 4 runs 28 ms eager against the 33 ms of Python it takes to enqueue); at 256 x 256 x 32 the GPU is the
        bound either way.  The first calls run eagerly (warm-up), the tensors in the returned `visuals` are overwritten by the
        next call, and the data-parallel exchange keeps the eager path.  defer_scalars: a replayed step returns a DeferredStep
        (`.result()` gives the usual tuple) instead of waiting for its scalars — the host then enqueues the next step while
        this one runs.  A model with a paired step (AugmentedCycleGAN.supervised_train_instance) replays that one from a
        second graph (`_sup_step_graph`) in the same way."""
        self._step_graph = StepGraph(self) if on else None
        self._sup_step_graph = None
        if on and hasattr(self, "_supervised_train_instance"):
            self._sup_step_graph = StepGraph(self, "_supervised_train_instance")
        for sg in (self._step_graph, self._sup_step_graph):
            if sg is not None:
                sg.defer_scalars = bool(defer_scalars)

    # ---- averaged generator weights (--ema_decay; no reference counterpart) ---------------------
    # An exponential moving average of the parameters of the generator-side networks (EMA_NETS), kept in FlatNet.ema by the
    # optimiser step (ops.ema_multi behind the Adam launch).  BatchNorm running buffers are not averaged: they are themselves
    # running averages of the live network's statistics, and the averaged model uses them as they are.
    _ema = ()              # [(checkpoint key of the network, its FlatNet)] of a model built with opt.ema_decay > 0
    _ema_active = False    # inside ema_weights(): `p` holds the averages and `ema` the live parameters

    def _setup_ema(self):
        """called once the optimisers exist; 0 for options written before the averaging existed (opt.pkl)"""
        d = float(getattr(self.opt, 'ema_decay', 0.0) or 0.0)
        if not 0.0 <= d < 1.0:
            raise ValueError("ema_decay must lie in [0, 1) (got %r)" % d)
        if d == 0.0:
            return
        flats = {id(f.net): f for opt in self._optimizers().values() for f in opt.flats}
        self._ema = [(k, flats[id(n)]) for k, n in self._net_dict().items() if k in self.EMA_NETS]
        for _, f in self._ema:
            f.enable_ema()
        for opt in self._optimizers().values():
            opt.ema_decay = d

    def _swap_ema(self):
        ops.swap_multi([(f.p, f.ema) for _, f in self._ema])
        for _, f in self._ema:     # the packed convolution weights follow in place: a captured step graph stays valid
            repack(f.net)

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the block the averaged networks run on their averaged parameters (one ops.swap_multi over their flat buffers
        and a repack per network on entry, the same on exit), so every forward-only method and metric scores the average.
        RuntimeError: a model without averages, a nested entry, and a training step or load() inside the block."""
        if not self._ema:
            raise RuntimeError("ema_weights: this model keeps no averaged weights (ema_decay is 0)")
        if self._ema_active:
            raise RuntimeError("ema_weights: already inside the block")
        self._swap_ema()
        self._ema_active = True
        try:
            yield self
        finally:
            self._ema_active = False
            self._swap_ema()

    def _live_only(self, what):
        if self._ema_active:
            raise RuntimeError("%s inside ema_weights(): the networks hold the averaged parameters" % what)

    @staticmethod
    def _state_dict_from(f, flat):
        """f.net.state_dict() with every parameter (under each of its keys) taken from `flat`, a buffer laid out as f.p; the
        buffers of the network as they are"""
        at = {f.p.data_ptr() + 4 * o: (o, p.numel()) for p, o in zip(f.params, f.offs)}
        out = OrderedDict()
        for k, v in f.net.state_dict().items():
            hit = at.get(v.data_ptr())
            out[k] = flat[hit[0]:hit[0] + hit[1]].view(v.shape) if hit is not None else v
        return out

    # ---- forward-only helpers shared by both models (model.py:210-280, 606-733): compositions of the two generators.
    # Subclass hooks: _z (noise transform), _cycle_code (the latent the B -> A -> B cycle is closed with).
    def _draw_prior(self, like):
        return like.new_empty((like.size(0), self.opt.nlatent, 1, 1)).normal_(0, 1)

    def predict_A(self, real_B):
        return self.netG_B_A.forward(real_B)

    def predict_B(self, real_A, z_B):
        return self.netG_A_B.forward(real_A, self._z(z_B))

    def generate_cycle(self, real_A, real_B, prior_z_B):
        fake_B, fake_A = self.predict_B(real_A, prior_z_B), self.predict_A(real_B)
        rec_A = self.predict_A(fake_B)
        rec_B = self.netG_A_B.forward(fake_A, self._cycle_code(fake_A, real_B, prior_z_B))
        return OrderedDict([('real_A', real_A.data), ('fake_B', fake_B.data), ('rec_A', rec_A.data),
                            ('real_B', real_B.data), ('fake_A', fake_A.data), ('rec_B', rec_B.data)])

    def generate_multi(self, real_A, multi_prior_z_B):
        """each A against multi_prior_z_B.size(0) / |A| consecutive codes (train.py:66)"""
        return self.predict_B(_each_n_times(real_A, multi_prior_z_B.size(0) // real_A.size(0)), multi_prior_z_B)

    def ensemble_groups(self, real_A, z, M, per):
        """The member loop of every translate_* method, a plain generator -> (g0, n, members): for inputs g0 .. g0 + n - 1
        (n <= per whole inputs, plan_ensemble) the n*M translations as forward_nhwc gives them, NHWC, member m of input i at
        row (i - g0)*M + m, made from rows i*M + m of z passed through _z (cycle_gan: a degenerate ensemble).  It keeps no
        state of its own to undo: the caller iterates it inside `with eval_state(self.netG_A_B), torch.no_grad():`, so a
        consumer that raises between two groups still leaves the flags and the grad mode as they were."""
        G = self.netG_A_B
        img_in = _starts_with_conv(G.model)
        for g0 in range(0, real_A.size(0), per):
            a = real_A[g0:g0 + per]
            n = a.size(0)
            x = ops.ToNHWC.apply(a.unsqueeze(1).expand(n, M, *a.shape[1:]).reshape(n * M, *a.shape[1:]), img_in)
            yield g0, n, G.forward_nhwc(x, as_latent(self._z(z[g0 * M:(g0 + n) * M])))

    def _groups(self, real_A, z, M, per, real_B=None):
        """ensemble_groups for the translate_* methods that write slices of whole-batch outputs -> (members, g), g the
        _Group of the inputs the members belong to; the paired real_B is detached and made contiguous once, here.  Stateless
        as ensemble_groups is: the caller holds eval_state and no_grad."""
        if real_B is not None:
            real_B = real_B.detach().contiguous()
        for g0, n, members in self.ensemble_groups(real_A, z, M, per):
            yield members, _Group(g0, n, M, real_B)

    def translate_ensemble(self, real_A, n_samples, z=None, real_B=None, quantiles=(0.05, 0.5, 0.95), chunk=None, cell_stats=None):
        """The distribution of A -> B: n_samples translations of every input, summarised per pixel on the device.
        z: (N*n_samples, nlatent, 1, 1) codes in generate_multi's order (input n takes rows n*M .. n*M + M - 1; default N(0, 1)
        from torch's generator); chunk: the most images one generator pass may hold (default: ensemble_chunk).  Arguments are
        settled by plan_ensemble and the members come group by group from ensemble_groups, in eval state under no_grad; each
        group is followed by one acg_ensemble_stats launch into slices of the outputs.  Returns device tensors: mean, std
        (N, C, H, W) and quantiles (N, nq, C, H, W); with real_B also the per-input crps, crps_fair (NaN for one sample),
        mse_mean, spread, coverage (N,), rank_hist (N, M + 1) and crps_map (N, C, H, W).  Nothing is read back to the host.
        cell_stats: None, or a record (state, thresholds, edges) of ops.cell_state and the tables ops.cell_stats takes (real_B
        required): each group's ensemble_stats launch is followed by one ops.cell_stats launch that adds the same members
        against the same NHWC truth to the state, per cell of the grid across the inputs, in input order.  No generator pass
        and no random draw of its own; what is returned keeps its bits."""
        if cell_stats is not None and real_B is None:
            raise ValueError("translate_ensemble: cell_stats needs the paired real_B")
        M, N, C, H, W, z, per = plan_ensemble("translate_ensemble", self.opt, real_A, n_samples, z, real_B, chunk,
                                              need_B=cell_stats is not None)
        q = ops.check_quantiles(quantiles)
        out = ops.ensemble_outputs(N, M, C, H, W, len(q), real_B is not None, real_A.device)
        with eval_state(self.netG_A_B), torch.no_grad():
            for g0, n, members in self.ensemble_groups(real_A, z, M, per):
                tgt = None
                if real_B is not None:
                    tgt = ops.ToNHWC.apply(real_B[g0:g0 + n], members.shape[-1] == ops.cimg(C))
                ops.ensemble_stats(members, tgt, M, C, q, out={k: v[g0:g0 + n] for k, v in out.items()})
                if cell_stats is not None:
                    state, thr, edges = cell_stats
                    ops.cell_stats(members, tgt, C, "nhwc", "nhwc", state, thresholds=thr, edges=edges, x_per_y=M)
        if real_B is None:
            return out
        sums, cells = out.pop("sums"), float(C * H * W)
        e1, e2 = sums[:, 0], sums[:, 1]
        out["crps"] = (e1 - e2 / 2) / cells
        out["crps_fair"] = (e1 - e2 * (M / (2. * (M - 1)))) / cells if M > 1 else torch.full_like(e1, float("nan"))
        out["mse_mean"] = sums[:, 2] / cells
        out["spread"] = torch.sqrt(sums[:, 3] / cells)
        out["coverage"] = sums[:, 4] / cells
        return out

    def translate_cell_stats_A(self, real_B, real_A, state, thresholds, edges, chunk=None):
        """B -> A per cell of the grid: the deterministic netG_B_A's translation of every real_B against the paired real_A,
        added to a state of ops.cell_state with M = 1 (ops.cell_stats; thresholds, edges as it takes them), in eval state under
        no_grad, in groups of at most `chunk` inputs (default ensemble_chunk), in input order -> the state.  ValueError for a
        real_A that does not pair.  Nothing is read back to the host."""
        if real_A.dim() != 4 or real_B.dim() != 4 or real_A.size(0) != real_B.size(0) or real_A.shape[2:] != real_B.shape[2:]:
            raise ValueError("translate_cell_stats_A: real_A %s does not pair with real_B %s" % (tuple(real_A.shape), tuple(real_B.shape)))
        chunk = ensemble_chunk(self.opt.ngf, real_B.size(2), real_B.size(3)) if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError("translate_cell_stats_A: chunk must be positive (got %d)" % chunk)
        real_A = real_A.detach().contiguous()
        with eval_state(self.netG_B_A), torch.no_grad():
            for g0 in range(0, real_B.size(0), chunk):
                pred = self.predict_A(real_B[g0:g0 + chunk])
                ops.cell_stats(pred, real_A[g0:g0 + chunk], real_A.size(1), "nchw", "nchw", state, thresholds=thresholds, edges=edges)
        return state

    def translate_spectrum(self, real_A, n_samples, z=None, real_B=None, chunk=None):
        """The variance of A -> B at every spatial scale: the radially averaged power spectrum (ops.radial_spectrum) of each
        of n_samples translations of every input and of their per-pixel mean (_ensemble_mean).  z, chunk and the refusals:
        plan_ensemble; the members: ensemble_groups.  Square fields of a power of two (ops.radial_spectrum's rule).  Returns
        device tensors: members (N, M, C, nb), ens_mean (N, C, nb) and with real_B also target (N, C, nb), nb = S/2 + 1.
        Nothing is read back to the host."""
        M, N, C, H, W, z, per = plan_ensemble("translate_spectrum", self.opt, real_A, n_samples, z, real_B, chunk)
        nb = ops._spectrum_size(H, W) // 2 + 1
        f = dict(device=real_A.device, dtype=torch.float32)
        out = dict(members=torch.empty((N, M, C, nb), **f), ens_mean=torch.empty((N, C, nb), **f))
        with eval_state(self.netG_A_B), torch.no_grad():
            for members, g in self._groups(real_A, z, M, per):
                ops.radial_spectrum(members, C, "nhwc", out=g.flat(out["members"]))
                ops.radial_spectrum(_ensemble_mean(members, M, C), C, "nchw", out=g.rows(out["ens_mean"]))
            if real_B is not None:
                out["target"] = ops.radial_spectrum(real_B, C, "nchw")
        return out

    def translate_coherence(self, real_A, n_samples, real_B, z=None, chunk=None):
        """Whether the variance of A -> B is in the right place: the paired cross-spectra (ops.cross_spectrum: per ring the
        means of Pxx, Pyy and the co-spectrum Cxy, x the translation, y the paired real_B) of each of n_samples translations
        of every input, one truth per M members, and of their per-pixel mean (_ensemble_mean).  z, chunk and the refusals:
        plan_ensemble, real_B required; the members: ensemble_groups.  Sizes as for translate_spectrum.  Returns device
        tensors: members (N, M, C, 3, nb) and ens_mean (N, C, 3, nb), nb = S/2 + 1, to be summed over a set of pairs and handed
        to ops.coherence_summary.  Nothing is read back to the host."""
        M, N, C, H, W, z, per = plan_ensemble("translate_coherence", self.opt, real_A, n_samples, z, real_B, chunk, need_B=True)
        nb = ops._spectrum_size(H, W) // 2 + 1
        f = dict(device=real_A.device, dtype=torch.float32)
        out = dict(members=torch.empty((N, M, C, 3, nb), **f), ens_mean=torch.empty((N, C, 3, nb), **f))
        with eval_state(self.netG_A_B), torch.no_grad():
            for members, g in self._groups(real_A, z, M, per, real_B):
                ops.cross_spectrum(members, g.b, C, "nhwc", "nchw", x_per_y=M, out=g.flat(out["members"]))
                ops.cross_spectrum(_ensemble_mean(members, M, C), g.b, C, "nchw", "nchw", out=g.rows(out["ens_mean"]))
        return out

    def translate_ssim(self, real_A, n_samples, real_B, z=None, chunk=None):
        """The local structure of A -> B: the structural similarity (ops.ssim: per channel the mean S and the mean
        contrast-structure factor cs, x the translation, y the paired real_B) of each of n_samples translations of every input,
        one truth per M members, and of their per-pixel mean (_ensemble_mean): the mean of an ensemble is smoother than any
        member, so it scores a higher luminance term and a lower cs.  z, chunk and the refusals: plan_ensemble, real_B
        required; the members: ensemble_groups.  11 <= H, W <= 1024.  Returns device tensors: members (N, M, C, 2) and
        ens_mean (N, C, 2).  Nothing is read back to the host."""
        M, N, C, H, W, z, per = plan_ensemble("translate_ssim", self.opt, real_A, n_samples, z, real_B, chunk, need_B=True)
        f = dict(device=real_A.device, dtype=torch.float32)
        out = dict(members=torch.empty((N, M, C, 2), **f), ens_mean=torch.empty((N, C, 2), **f))
        with eval_state(self.netG_A_B), torch.no_grad():
            for members, g in self._groups(real_A, z, M, per, real_B):
                ops.ssim(members, g.b, C, "nhwc", "nchw", x_per_y=M, out=g.flat(out["members"]))
                ops.ssim(_ensemble_mean(members, M, C), g.b, C, "nchw", "nchw", out=g.rows(out["ens_mean"]))
        return out

    def translate_marginal(self, real_A, n_samples, real_B, levels, edges, z=None, chunk=None):
        """Whether A -> B has the right values: per channel the Wasserstein distances w1 and w2sq of the value distribution of
        a field against that of its paired real_B, its quantiles at `levels` and its counts of values below `edges`
        (ops.sorted_scores on ops.field_sort's sorted fields), of each of n_samples translations of every input, one truth per
        M members, of their per-pixel mean (_ensemble_mean: smoother than any member, so its tails are short) and, without a
        distance, of the truth itself.  Per group the truth is sorted once and shared by the member and the ensemble-mean call.
        levels: at most 16 inside [0, 1] (ops.check_levels); edges: (C, E), E <= 256, moved to the device once; at least one
        of each.  z, chunk and the refusals: plan_ensemble, real_B required; the members: ensemble_groups.  H W <= 2^20.
        Returns device tensors, w float64, q float32, below int32: members = dict(w (N, M, C, 2), q (N, M, C, L), below
        (N, M, C, E)), ens_mean = dict(w (N, C, 2), q (N, C, L), below (N, C, E)) and target = dict(q (N, C, L), below
        (N, C, E)).  Nothing is read back to the host."""
        M, N, C, H, W, z, per = plan_ensemble("translate_marginal", self.opt, real_A, n_samples, z, real_B, chunk, need_B=True)
        lv = ops.check_levels(levels)
        if not lv:
            raise ValueError("translate_marginal: need 1..%d levels (got none)" % ops.MARG_MAX_LEVELS)
        e = ops.channel_table("translate_marginal", ValueError, "edges", edges, C, ops.MARG_MAX_EDGES, real_A.device, cast=True)
        L, E = len(lv), e.size(1)
        dev = real_A.device

        def outputs(lead, w):
            o = dict(q=torch.empty(lead + (C, L), device=dev, dtype=torch.float32),
                     below=torch.empty(lead + (C, E), device=dev, dtype=torch.int32))
            if w:
                o["w"] = torch.empty(lead + (C, 2), device=dev, dtype=torch.float64)
            return o
        out = dict(members=outputs((N, M), True), ens_mean=outputs((N,), True), target=outputs((N,), False))
        with eval_state(self.netG_A_B), torch.no_grad():
            for members, g in self._groups(real_A, z, M, per, real_B):
                sb, _ = ops.field_sort(g.b, C, "nchw", want_rank=False)
                sm, _ = ops.field_sort(members, C, "nhwc", want_rank=False)
                ops.sorted_scores(sm, sb, lv, e, x_per_y=M, out={k: g.flat(v) for k, v in out["members"].items()})
                se, _ = ops.field_sort(_ensemble_mean(members, M, C), C, "nchw", want_rank=False)
                ops.sorted_scores(se, sb, lv, e, out={k: g.rows(v) for k, v in out["ens_mean"].items()})
                ops.sorted_scores(sb, None, lv, e, out={k: g.rows(v) for k, v in out["target"].items()})
        return out

    def translate_fss(self, real_A, n_samples, real_B, thresholds, windows, z=None, chunk=None, scales=False, reliability=None):
        """Whether A -> B puts its threshold exceedances close enough: the fractions-skill-score triples (ops.fss: per
        channel, threshold and window the sums of cf^2, co^2 and cf co of the window counts of the events, x the translation,
        y the paired real_B) of each of n_samples translations of every input, of the ensemble as a probability (the summed
        counts of the M members of an input, the same ops.fss call with x_per_y = M) and of their per-pixel mean
        (_ensemble_mean).  thresholds: (C, T), moved to the device once; windows: odd widths, as ops.fss takes them.  z,
        chunk and the refusals: plan_ensemble, real_B required; the members: ensemble_groups.  Any H x W the generator
        accepts.  Returns int64 device tensors: members (N, M, C, T, nw, 3), ens_prob (N, C, T, nw, 3) and ens_mean
        (N, C, T, nw, 3), to be summed over a set of pairs and handed to ops.fss_summary (ens_prob with members=M).
        scales=True: the intensity-scale triples of the same events too (ops.fss_scales, nl = ops.fss_scale_levels(H, W)
        dyadic levels in place of the windows), of the same members in the same group loop, as members_scale
        (N, M, C, T, nl, 3), ens_prob_scale and ens_mean_scale (N, C, T, nl, 3), for ops.fss_scale_summary; with False
        neither the entries nor their launches exist.  reliability: None, or a tuple of odd windows of at most 65
        (ops.check_rel_windows): the reliability tables of the same events too (ops.reliability: cells by the number of members
        in the neighbourhood event and by the truth's), of the same members in the same group loop with no random draw of
        their own, as ens_rel (N, C, T, nwr, M + 1, 2) of the ensemble (x_per_y = M), members_rel (N, M, C, T, nwr, 2, 2) and
        ens_mean_rel (N, C, T, nwr, 2, 2) of single fields, for ops.reliability_summary; with None neither the entries nor
        their launches exist.  Nothing is read back to the host."""
        M, N, C, H, W, z, per = plan_ensemble("translate_fss", self.opt, real_A, n_samples, z, real_B, chunk, need_B=True)
        win = ops.check_windows(windows)
        thr = ops.channel_table("translate_fss", ValueError, "thresholds", thresholds, C, ops.FSS_MAX_T, real_A.device, cast=True)
        T, nw = thr.size(1), len(win)
        i64 = dict(device=real_A.device, dtype=torch.int64)
        out = dict(members=torch.empty((N, M, C, T, nw, 3), **i64), ens_prob=torch.empty((N, C, T, nw, 3), **i64),
                   ens_mean=torch.empty((N, C, T, nw, 3), **i64))
        if scales:
            nl = ops.fss_scale_levels(H, W)
            out.update(members_scale=torch.empty((N, M, C, T, nl, 3), **i64), ens_prob_scale=torch.empty((N, C, T, nl, 3), **i64),
                       ens_mean_scale=torch.empty((N, C, T, nl, 3), **i64))
        if reliability is not None:
            rwin = ops.check_rel_windows(reliability)
            nwr = len(rwin)
            out.update(ens_rel=torch.empty((N, C, T, nwr, M + 1, 2), **i64), members_rel=torch.empty((N, M, C, T, nwr, 2, 2), **i64),
                       ens_mean_rel=torch.empty((N, C, T, nwr, 2, 2), **i64))
        with eval_state(self.netG_A_B), torch.no_grad():
            for members, g in self._groups(real_A, z, M, per, real_B):
                ops.fss(members, g.b, C, "nhwc", "nchw", thr, win, x_per_y=M, ensemble=True,
                        out=(g.flat(out["members"]), g.rows(out["ens_prob"])))
                mean = _ensemble_mean(members, M, C)
                ops.fss(mean, g.b, C, "nchw", "nchw", thr, win, out=g.rows(out["ens_mean"]))
                if scales:
                    ops.fss_scales(members, g.b, C, "nhwc", "nchw", thr, x_per_y=M, ensemble=True,
                                   out=(g.flat(out["members_scale"]), g.rows(out["ens_prob_scale"])))
                    ops.fss_scales(mean, g.b, C, "nchw", "nchw", thr, out=g.rows(out["ens_mean_scale"]))
                if reliability is not None:
                    ops.reliability(members, g.b, C, "nhwc", "nchw", thr, rwin, x_per_y=M, out=g.rows(out["ens_rel"]))
                    ops.reliability(members, _each_n_times(g.b, M), C, "nhwc", "nchw", thr, rwin,   # a table per member: a truth row each
                                    out=g.flat(out["members_rel"]))
                    ops.reliability(mean, g.b, C, "nchw", "nchw", thr, rwin, out=g.rows(out["ens_mean_rel"]))
        return out

    def translate_minkowski(self, real_A, n_samples, thresholds, z=None, chunk=None, components=0):
        """The shape of what A -> B puts above a threshold: the counts behind the Minkowski functionals (ops.minkowski: per
        channel and threshold nF, nE1, nE2, nV1, nV4 of the excursion set, from which ops.minkowski_summary takes area,
        perimeter and the two Euler numbers) of each of n_samples translations of every input and of their per-pixel mean
        (_ensemble_mean: smoother than any member, so it has fewer, rounder objects).  Unpaired: no real_B; the real fields
        go through ops.minkowski themselves.  thresholds: (C, T), 1 <= T <= 255, per channel finite and non-decreasing; a
        host array is checked (ops.channel_table) and moved to the device once, a device tensor is taken as it is.  z,
        chunk and the refusals: plan_ensemble; the members: ensemble_groups.  1 <= H, W <= 1024.  Returns int64 device
        tensors: members (N, M, C, T, 5) and ens_mean (N, C, T, 5), to be summed over a set of fields and handed to
        ops.minkowski_summary.  components: 0, or the connectivity 4 or 8: the connected components of the same sets
        (ops.components: n, area, sum of squared areas, n_border and the 21 size bins) of the same members and of their mean,
        in the same group loop, as members_comp (N, M, C, T, 25) and ens_mean_comp (N, C, T, 25), for
        ops.components_summary; with 0 neither the entries nor their launches exist.  Nothing is read back to the host."""
        if components not in (0, 4, 8):
            raise ValueError("translate_minkowski: components must be 0, 4 or 8 (got %r)" % (components,))
        M, N, C, H, W, z, per = plan_ensemble("translate_minkowski", self.opt, real_A, n_samples, z, None, chunk)
        thr = ops.channel_table("translate_minkowski", ValueError, "thresholds", thresholds, C, ops.MINK_MAX_T, real_A.device,
                                ordered=True, cast=True)
        T = thr.size(1)
        i64 = dict(device=real_A.device, dtype=torch.int64)
        out = dict(members=torch.empty((N, M, C, T, 5), **i64), ens_mean=torch.empty((N, C, T, 5), **i64))
        if components:
            out.update(members_comp=torch.empty((N, M, C, T, ops.COMP_STATS), **i64),
                       ens_mean_comp=torch.empty((N, C, T, ops.COMP_STATS), **i64))
        with eval_state(self.netG_A_B), torch.no_grad():
            for members, g in self._groups(real_A, z, M, per):
                ops.minkowski(members, C, "nhwc", thr, out=g.flat(out["members"]))
                mean = _ensemble_mean(members, M, C)
                ops.minkowski(mean, C, "nchw", thr, out=g.rows(out["ens_mean"]))
                if components:
                    ops.components(members, C, "nhwc", thr, conn=components, out=g.flat(out["members_comp"]))
                    ops.components(mean, C, "nchw", thr, conn=components, out=g.rows(out["ens_mean_comp"]))
        return out

    def translate_sal(self, real_A, n_samples, real_B, thresholds, floor=-1.0, conn=8, z=None, chunk=None):
        """Whether the objects of A -> B are too large and flat or too small and peaked, carry too much of the quantity, or lie
        in the wrong place: the weighted moments behind the SAL score (ops.sal: per channel the mass sums Q, QY, QX of the
        field and, per threshold, n, area, Robj, Rmax and the double sums SV, SR of the objects of the excursion set) of each
        of n_samples translations of every input, of their per-pixel mean (_ensemble_mean: smoother than any member, so its
        structure score is positive) and of the paired real_B.  thresholds: (C, T), 1 <= T <= 255, per channel finite and
        non-decreasing; a host array is checked (ops.channel_table) and moved to the device once.  floor: finite, the lower end
        of the data range; conn: 4 or 8.  z, chunk and the refusals: plan_ensemble, real_B required; the members:
        ensemble_groups.  1 <= H, W <= 1024.  Returns device tensors, * = field (.., C, 3) int64, obj (.., C, T, 4) int64 and
        shape (.., C, T, 2) float64: members_* (N, M, ..), ens_mean_* (N, ..) and target_* (N, ..), for ops.sal_scores
        (members (N, M, ..) against target[:, None]).  Nothing is read back to the host."""
        M, N, C, H, W, z, per = plan_ensemble("translate_sal", self.opt, real_A, n_samples, z, real_B, chunk, need_B=True)
        thr = ops.channel_table("translate_sal", ValueError, "thresholds", thresholds, C, ops.MINK_MAX_T, real_A.device,
                                ordered=True, cast=True)
        T = thr.size(1)
        parts = (("field", (C, 3), torch.int64), ("obj", (C, T, 4), torch.int64), ("shape", (C, T, 2), torch.float64))
        out = {}
        for who, lead in (("members", (N, M)), ("ens_mean", (N,)), ("target", (N,))):
            for name, shape, dtype in parts:
                out["%s_%s" % (who, name)] = torch.empty(lead + shape, device=real_A.device, dtype=dtype)
        triple = lambda who, view: tuple(view(out["%s_%s" % (who, name)]) for name, _, _ in parts)
        with eval_state(self.netG_A_B), torch.no_grad():
            for members, g in self._groups(real_A, z, M, per, real_B):
                ops.sal(members, C, "nhwc", thr, floor=floor, conn=conn, out=triple("members", g.flat))
                ops.sal(_ensemble_mean(members, M, C), C, "nchw", thr, floor=floor, conn=conn, out=triple("ens_mean", g.rows))
                ops.sal(g.b, C, "nchw", thr, floor=floor, conn=conn, out=triple("target", g.rows))
        return out

    def _field_groups(self, who, G, x, copies, C, overlap, chunk, code=None):
        """What translate_field and translate_field_A share -> (copies*N, C, H, W): every (N, Cin, H, W) field of x, `copies`
        times in a row, through G in windows of grid_size (ops.window_plan) blended on canvases (ops.window_blend).  Groups
        hold whole canvases: T = ny*nx windows each, at most chunk // T canvases per pass; canvas k of a group is cut
        (ops.window_gather) from field k // copies, tile (ky, kx) at row (k*ny + ky)*nx + kx.  code(k0, n): the latent rows
        of canvases k0 .. k0 + n - 1, one each, repeated here for the T windows of a canvas."""
        S = int(self.opt.grid_size)
        if x.dim() != 4 or x.size(2) < S or x.size(3) < S:
            raise ValueError("%s: fields %s are smaller than the %d x %d window (grid_size)" % (who, tuple(x.shape), S, S))
        N, _, H, W = x.shape
        plan = ops.window_plan(H, W, S, S // 4 if overlap is None else overlap)
        T = plan.ny * plan.nx
        chunk = ensemble_chunk(self.opt.ngf, S, S) if chunk is None else int(chunk)
        per = chunk // T
        if per < 1:
            raise ValueError("%s: a group of %d images cannot hold the %d windows of one %d x %d field" % (who, chunk, T, H, W))
        x = x.detach()
        out = torch.empty((N * copies, C, H, W), device=x.device, dtype=torch.float32)
        win = [(oy, ox, 0) for oy in plan.oy[:plan.ny] for ox in plan.ox[:plan.nx]]
        img_in = _starts_with_conv(G.model)
        with eval_state(G), torch.no_grad():
            for k0 in range(0, N * copies, per):
                n = min(per, N * copies - k0)
                tiles = ops.window_gather(x, [(k // copies,) + w for k in range(k0, k0 + n) for w in win], S, img=img_in)
                if code is None:
                    y = G.forward_nhwc(tiles)
                else:
                    y = G.forward_nhwc(tiles, as_latent(code(k0, n)).repeat_interleave(T, dim=0))
                ops.window_blend(y, plan, n, C, out=out[k0:k0 + n])
        return out

    def translate_field(self, real_A, n_samples=1, z=None, overlap=None, chunk=None):
        """A -> B on fields of any H x W >= grid_size at their own resolution -> (N, M, C_out, H, W) on the device: every
        field is cut into overlapping grid_size windows (ops.window_plan; overlap defaults to grid_size // 4), the windows
        go through netG_A_B as they would in training, and the translations are blended at the seams with a linear ramp
        (ops.window_blend).  One code per (field, member), shared by all windows of that member: z is (N*M, nlatent, 1, 1) in
        generate_multi's order, drawn as in plan_ensemble when absent.  chunk: the most windows one generator pass may hold
        (default ensemble_chunk at the window size); ValueError if one field's windows do not fit, for a field below
        grid_size, n_samples outside 1..ops.ENSEMBLE_MAX_M and a wrong number of codes.  For H = W = grid_size this is
        predict_B, bit for bit.  Eval state under no_grad, both restored; nothing is kept, nothing is read back."""
        M = int(n_samples)
        if not 1 <= M <= ops.ENSEMBLE_MAX_M:
            raise ValueError("translate_field: n_samples must lie in 1..%d (got %d)" % (ops.ENSEMBLE_MAX_M, M))
        N = real_A.size(0)
        if z is None:
            z = real_A.new_empty((N * M, self.opt.nlatent, 1, 1)).normal_(0, 1)
        if z.size(0) != N * M:
            raise ValueError("translate_field: z holds %d codes for %d fields x %d samples" % (z.size(0), N, M))
        out = self._field_groups("translate_field", self.netG_A_B, real_A, M, self.opt.output_nc, overlap, chunk,
                                 code=lambda k0, n: self._z(z[k0:k0 + n]))
        return out.view(N, M, *out.shape[1:])

    def translate_field_A(self, real_B, overlap=None, chunk=None):
        """B -> A on fields of any H x W >= grid_size -> (N, C_in, H, W): translate_field's windows and blend through the
        deterministic netG_B_A; for H = W = grid_size this is predict_A, bit for bit."""
        return self._field_groups("translate_field_A", self.netG_B_A, real_B, 1, self.opt.input_nc, overlap, chunk)

    def translate_field_spectrum(self, real_A, n_samples, real_B, z=None, overlap=None, chunk=None):
        """translate_coherence for whole fields: the paired cross-spectra (ops.field_cross_spectrum: per elliptical ring the
        means of Pxx, Pyy and Cxy, x the translation, y the paired whole real_B) of each of n_samples tiled translations of
        every field (translate_field: z, overlap, chunk and the refusals are its own) and of their per-pixel mean
        (_ensemble_mean).  Any H x W >= grid_size with both extents in 16 .. 1024; real_B is required and has the fields'
        H x W.  This is where seams (power at the window pitch) and the blend ramp (lost small-scale variance) show.  Returns
        device tensors: members (N, M, C, 3, nb) and ens_mean (N, C, 3, nb), nb = min(H, W) // 2 + 1, to be summed over a set
        of pairs and handed to ops.coherence_summary; Pxx and Pyy are the plain spectra.  For H = W = grid_size a power of two
        this is translate_coherence, bit for bit.  Nothing is read back to the host."""
        C = self.opt.output_nc
        if real_B is None or real_B.dim() != 4 or real_A.dim() != 4 or \
                tuple(real_B.shape) != (real_A.size(0), C) + tuple(real_A.shape[2:]):
            raise ValueError("translate_field_spectrum: real_B %s does not pair with real_A %s"
                             % (None if real_B is None else tuple(real_B.shape), tuple(real_A.shape)))
        fields = self.translate_field(real_A, n_samples, z=z, overlap=overlap, chunk=chunk)
        N, M, _, H, W = fields.shape
        members = fields.view(N * M, C, H, W)
        real_B = real_B.detach().contiguous()
        with torch.no_grad():
            out = dict(members=ops.field_cross_spectrum(members, real_B, C, "nchw", "nchw", x_per_y=M))
            out["members"] = out["members"].view(N, M, C, 3, -1)
            mean = _ensemble_mean(ops.ToNHWC.apply(members, True), M, C)
            out["ens_mean"] = ops.field_cross_spectrum(mean, real_B, C, "nchw", "nchw")
        return out

    def generate_cycle_B_multi(self, real_B, multi_prior_z_B):
        fake_A = self.predict_A(real_B)
        return fake_A, self.netG_A_B.forward(_each_n_times(fake_A, multi_prior_z_B.size(0) // real_B.size(0)), multi_prior_z_B)

    def generate_noisy_cycle(self, real_B, std):
        """B -> A, perturb A by N(0, std/127.5) (clamped to the image range), -> B"""
        fake_A = self.predict_A(real_B)
        perturb = lambda: torch.clamp(fake_A + torch.empty_like(fake_A).normal_(0, std / 127.5), -1, 1)
        if self._noise_before_code:     # order of the random draws as in the reference (model.py:626-645 vs 257-266)
            noisy, code = perturb(), self._cycle_code(fake_A, real_B, None)
        else:
            code, noisy = self._cycle_code(fake_A, real_B, None), perturb()
        return self.netG_A_B.forward(noisy, code)

    def generate_multi_cycle(self, real_B, steps):
        images, B = [real_B.data], real_B
        for _ in range(steps):
            A = self.predict_A(B)
            B = self.netG_A_B.forward(A, self._z(self._draw_prior(real_B)))
            images += [A.data, B.data]
        return images

    # ---- north-star aliases -----------------------------------------------------
    def set_input(self, data, prior_z_B=None):
        self._input = (data['A'], data['B'], prior_z_B)

    def optimize_parameters(self):
        A, B, z = self._input
        if z is None:
            z = torch.randn(A.size(0), self.opt.nlatent, 1, 1, device=A.device)
        self._last = self.train_instance(A, B, z)
        return self._last

    def eval(self):
        for n in self._nets():
            n.eval()

    def train(self):
        for n in self._nets():
            n.train()


@contextlib.contextmanager
def _in_train_step():
    """SyncBN collectives are issued only inside a training step, where every rank runs the same forward/backward; the
    rank-0-only forwards of train.py (visualisation, evaluation) then use local statistics instead of posting
    collectives the other ranks never join."""
    from . import modules
    prev, modules.IN_TRAIN_STEP = modules.IN_TRAIN_STEP, True
    try:
        yield
    finally:
        modules.IN_TRAIN_STEP = prev


def ensemble_chunk(ngf, H, W):
    """the largest number of images one generator pass may hold: its widest full-resolution tensor (2*ngf channels, stored
    as cpad) must stay under the 4 GiB operand limit of every launcher — 255 images at 256 x 256 and 63 at
    512 x 512 with ngf 32"""
    per_image = H * W * ops.cpad(2 * ngf) * 4
    return max(((1 << 32) - 1) // per_image, 1)


def plan_ensemble(who, opt, real_A, n_samples, z=None, real_B=None, chunk=None, need_B=False):
    """What every translate_* method settles before its generator runs -> (M, N, C, H, W, z, per): M samples of each of N
    inputs, the C x H x W of a translation, the (N*M, nlatent, 1, 1) codes (drawn here, once, from torch's generator when none
    are given) and `per`, the whole inputs of one group: chunk // M, chunk defaulting to ensemble_chunk.  ValueError (prefixed
    `who`) for n_samples outside 1..ops.ENSEMBLE_MAX_M, codes that do not count N*M, a real_B (required with need_B) that does
    not pair with real_A, and a chunk below M.  Shapes and Python only: no kernel, no device work beyond the draw."""
    M = int(n_samples)
    if not 1 <= M <= ops.ENSEMBLE_MAX_M:
        raise ValueError("%s: n_samples must lie in 1..%d (got %d)" % (who, ops.ENSEMBLE_MAX_M, M))
    N, _, H, W = real_A.shape
    C = opt.output_nc
    if z is None:
        z = real_A.new_empty((N * M, opt.nlatent, 1, 1)).normal_(0, 1)
    if z.size(0) != N * M:
        raise ValueError("%s: z holds %d codes for %d inputs x %d samples" % (who, z.size(0), N, M))
    if (need_B and real_B.dim() != 4) or (real_B is not None and (real_B.size(0), real_B.size(1)) != (N, C)):
        raise ValueError("%s: real_B %s does not pair with real_A %s" % (who, tuple(real_B.shape), tuple(real_A.shape)))
    chunk = ensemble_chunk(opt.ngf, H, W) if chunk is None else int(chunk)
    per = chunk // M
    if per < 1:
        raise ValueError("%s: a group of %d images cannot hold one input's %d samples" % (who, chunk, M))
    return M, N, C, H, W, z, per


@contextlib.contextmanager
def eval_state(net):
    """net.eval() inside the block, every module's own .training flag back on the way out; entered together with
    torch.no_grad() by whoever iterates _Base.ensemble_groups"""
    modes = [(m, m.training) for m in net.modules()]
    net.eval()
    try:
        yield net
    finally:
        for m, mode in modes:
            m.training = mode


class _Group(object):
    """Inputs g0 .. g0 + n - 1 of a batch, M members each, as a translate_* method addresses them: b, their rows of the
    paired real_B (None without one); rows(t) = t[g0:g0 + n] of a per-input tensor (N, ...); flat(t), the same rows of a
    per-member tensor (N, M, ...) as (n*M, ...), one row per member in ensemble_groups' order.  Views: kernels write into them."""

    def __init__(self, g0, n, M, real_B):
        self.g0, self.n, self.M = g0, n, M
        self.b = None if real_B is None else self.rows(real_B)

    def rows(self, t):
        return t[self.g0:self.g0 + self.n]

    def flat(self, t):
        return self.rows(t).view((self.n * self.M,) + tuple(t.shape[2:]))


def _ensemble_mean(members, M, C):
    """the per-pixel mean of every input's M members (NHWC) -> (n, C, H, W): acg_ensemble_stats writing its mean map alone"""
    mean = torch.empty((members.size(0) // M, C, members.size(1), members.size(2)), device=members.device, dtype=torch.float32)
    ops.ensemble_stats(members, None, M, C, (0.5,), out=dict(mean=mean))
    return mean


def _each_n_times(x, n):
    """(N, ...) -> (N*n, ...): every sample n times in a row"""
    return x.repeat_interleave(n, dim=0)


def _n_blocks(opt):
    from . import modules
    modules.SYNC_BN = bool(getattr(opt, 'sync_bn', False))   # extension: BatchNorm statistics over all ranks
    return int(getattr(opt, 'n_blocks', 3))


class StochCycleGAN(_Base):
    """Stochastic cycle gan — model.py:75-325"""

    def __init__(self, opt, ignore_noise=False, testing=False):
        self.ignore_noise = ignore_noise
        self._exchanges = {}
        self.old_lr = opt.lr
        opt.use_sigmoid = opt.no_lsgan
        self.opt = opt
        nb = _n_blocks(opt)
        self.netG_A_B = networks.define_stochastic_G(nlatent=opt.nlatent, input_nc=opt.input_nc, output_nc=opt.output_nc,
                                                     ngf=opt.ngf, which_model_netG=opt.which_model_netG, norm=opt.norm,
                                                     use_dropout=opt.use_dropout, gpu_ids=opt.gpu_ids, n_blocks=nb)
        self.netG_B_A = networks.define_G(input_nc=opt.output_nc, output_nc=opt.input_nc, ngf=opt.ngf,
                                          which_model_netG=opt.which_model_netG, norm=opt.norm,
                                          use_dropout=opt.use_dropout, gpu_ids=opt.gpu_ids, n_blocks=nb)
        self.netD_A = networks.define_D_A(input_nc=opt.input_nc, ndf=32, which_model_netD=opt.which_model_netD,
                                          norm=opt.norm, use_sigmoid=opt.use_sigmoid, gpu_ids=opt.gpu_ids)
        self.netD_B = networks.define_D_B(input_nc=opt.output_nc, ndf=opt.ndf, which_model_netD=opt.which_model_netD,
                                          norm=opt.norm, use_sigmoid=opt.use_sigmoid, gpu_ids=opt.gpu_ids)
        self._build_optimizers()
        # --no_lsgan: the reference binds its (broken) BCE branch here; the float-target fix
        self.criterionGAN = criterion_GAN_bce if opt.use_sigmoid else functools.partial(criterion_GAN, use_sigmoid=False)
        self.criterionCycle = lambda a, b: ops.L1.apply(_as2d(a), _as2d(b), a.shape[1])
        if not testing:
            with open("%s/nets.txt" % opt.expr_dir, 'w') as nets_f:
                for n in self._nets():
                    networks.print_network(n, nets_f)

    def _nets(self):
        return [self.netG_A_B, self.netG_B_A, self.netD_A, self.netD_B]

    def _build_optimizers(self):
        o = self.opt
        acg_dist.broadcast_params_(self._nets())
        self.f_G_A_B, self.f_G_B_A = FlatNet(self.netG_A_B), FlatNet(self.netG_B_A)
        self.f_D_A, self.f_D_B = FlatNet(self.netD_A), FlatNet(self.netD_B)
        self.optimizer_G = FusedAdam([self.f_G_A_B, self.f_G_B_A], o.lr, (o.beta1, 0.999))      # model.py:109-111
        self.optimizer_D = FusedAdam([self.f_D_A, self.f_D_B], o.lr / 5., (o.beta1, 0.999))     # model.py:112-114
        self._setup_ema()

    EMA_NETS = ('netG_A_B', 'netG_B_A')      # the networks of optimizer_G

    def train_instance(self, real_A, real_B, prior_z_B):
        self._live_only("train_instance")
        if self._step_graph is not None and not acg_dist.exchange_on():
            return self._step_graph(real_A, real_B, prior_z_B)
        with _in_train_step():
            return self._train_instance(real_A, real_B, prior_z_B)

    def _train_instance(self, real_A, real_B, prior_z_B):
        o = self.opt
        nA, nB = o.input_nc, o.output_nc
        for f in (self.f_G_A_B, self.f_G_B_A, self.f_D_A, self.f_D_B):
            f.check()
        if self.ignore_noise:
            prior_z_B = prior_z_B.mul(0.).add(1.)                                               # model.py:128-129
        A, B, z = ops.ToNHWC.apply(real_A, True), ops.ToNHWC.apply(real_B, True), as_latent(prior_z_B)
        fake_B = self.netG_A_B.forward_nhwc(A, z)
        fake_A = self.netG_B_A.forward_nhwc(B)

        # ---- D phase (model.py:139-162)
        p_fA = self.netD_A.forward_nhwc(fake_A.detach()); l_fA = self._gan_loss(p_fA, False)
        p_tA = self.netD_A.forward_nhwc(A); l_tA = self._gan_loss(p_tA, True)
        p_fB = self.netD_B.forward_nhwc(fake_B.detach()); l_fB = self._gan_loss(p_fB, False)
        p_tB = self.netD_B.forward_nhwc(B); l_tB = self._gan_loss(p_tB, True)
        loss_D_A, loss_D_B = 0.5 * (l_fA + l_tA), 0.5 * (l_fB + l_tB)
        loss_D = loss_D_A + loss_D_B
        self.optimizer_D.zero_grad()
        ex_D = self._backward(loss_D, "stoch.D", [self.f_D_B, self.f_D_A])    # D_B was built last: its backward runs first
        m_tA, m_tB = ops.mean_valid(p_tA, 1), ops.mean_valid(p_tB, 1)

        # ---- G phase (model.py:167-190).  The cycle forwards do not depend on the discriminators: they run while the
        # D gradients are being all-reduced; the D forwards wait for the UPDATED discriminators (model.py:164-166)
        rec_A = self.netG_B_A.forward_nhwc(fake_B); loss_cycle_A = ops.L1.apply(rec_A, A, nA)
        rec_B = self.netG_A_B.forward_nhwc(fake_A, z); loss_cycle_B = ops.L1.apply(rec_B, B, nB)
        self._wait(ex_D, self.f_D_A, self.f_D_B)
        ss_D_A, ss_D_B = self.optimizer_D.clip_and_step(o.max_gnorm)
        ss_D_A, ss_D_B = ss_D_A.clone(), ss_D_B.clone()
        self.f_D_A.set_requires_grad(False); self.f_D_B.set_requires_grad(False)   # D weight grads are not needed
        try:
            p_fA = self.netD_A.forward_nhwc(fake_A); loss_G_A = self._gan_loss(p_fA, True)
            p_fB = self.netD_B.forward_nhwc(fake_B); loss_G_B = self._gan_loss(p_fB, True)
            loss_G = loss_G_A + loss_G_B + loss_cycle_A * o.lambda_A + loss_cycle_B * o.lambda_B
            loss_G, opt_sums, opt_names = losses.add_terms(self, losses.UNPAIRED, loss_G, A, B, z,
                                                           fake=(fake_A, fake_B), rec=(rec_A, rec_B))
            self.optimizer_G.zero_grad()
            sums = [loss_D_A, loss_G_A, loss_cycle_A, loss_D_B, loss_G_B, loss_cycle_B,
                    m_tA, ops.mean_valid(p_fA, 1), m_tB, ops.mean_valid(p_fB, 1)] + opt_sums
            ex_G = self._backward(loss_G, "stoch.G", [self.f_G_B_A, self.f_G_A_B], tail=(self.f_G_A_B, sums))
        finally:
            self.f_D_A.set_requires_grad(True); self.f_D_B.set_requires_grad(True)
        self._wait(ex_G, self.f_G_A_B, self.f_G_B_A)
        ss_G_A_B, ss_G_B_A = self.optimizer_G.clip_and_step(o.max_gnorm)

        n_loss = len(sums)
        names = ['D_A', 'G_A', 'Cyc_A', 'D_B', 'G_B', 'Cyc_B', 'P_t_A', 'P_f_A', 'P_t_B', 'P_f_B'] + \
                opt_names + ['gnorm_G_A_B', 'gnorm_G_B_A', 'gnorm_D_B', 'gnorm_D_A']
        vals = self._scalars(ex_G, self.f_G_A_B, names, sums, local=[ss_G_A_B, ss_G_B_A, ss_D_B, ss_D_A])
        visuals = OrderedDict([('real_A', real_A.detach()), ('fake_B', self._nchw(fake_B, nB)),
                               ('rec_A', self._nchw(rec_A, nA)), ('real_B', real_B.detach()),
                               ('fake_A', self._nchw(fake_A, nA)), ('rec_B', self._nchw(rec_B, nB))])

        def finish(vals):
            losses = OrderedDict((k, vals[k]) for k in names[:n_loss])                           # model.py:193-196
            if o.monitor_gnorm:
                gnorms = OrderedDict((k, math.sqrt(max(vals[k], 0.0))) for k in names[n_loss:])  # model.py:202-205
                return losses, visuals, gnorms
            return losses, visuals
        return self._report(vals, finish)

    # ---- hooks of the shared forward-only helpers (_Base; model.py:210-280) -------------------
    _noise_before_code = False

    def _z(self, z):
        return z.mul(0.).add(1.) if self.ignore_noise else z                                     # model.py:128-129

    def _cycle_code(self, fake_A, real_B, prior_z_B):
        """the code the B -> A -> B cycle is closed with: no encoder here, the given prior"""
        return self._z(prior_z_B) if prior_z_B is not None else self._z(self._draw_prior(real_B))

    def _optimizers(self):
        return OrderedDict([('optimizer_D', self.optimizer_D), ('optimizer_G', self.optimizer_G)])

    def _net_dict(self):
        return OrderedDict([('netG_A_B', self.netG_A_B), ('netG_B_A', self.netG_B_A), ('netD_A', self.netD_A),
                            ('netD_B', self.netD_B)])

    def update_learning_rate(self):
        """model.py:282-291 (also overwrites the discriminators' lr/5 — reference behaviour)"""
        lrd = self.opt.lr / self.opt.niter_decay
        lr = self.old_lr - lrd
        for opt in self._optimizers().values():
            for param_group in opt.param_groups:
                param_group['lr'] = lr
        print('update learning rate: %f -> %f' % (self.old_lr, lr))
        self.old_lr = lr

    def save(self, chk_name):
        """model.py:293-303 / 750-764: same checkpoint keys, torch.load-able.  A model with averaged weights adds `ema_<net>`
        per averaged network (a full state_dict: the averaged parameters, the live buffers) and `ema_decay`; the reference's
        keys hold the live weights, inside ema_weights() too."""
        chk_path = os.path.join(self.opt.expr_dir, chk_name)
        checkpoint = {k: n.state_dict() for k, n in self._net_dict().items()}
        for k, f in self._ema:
            avg = self._state_dict_from(f, f.ema)      # inside ema_weights() the two buffers have changed places
            checkpoint[k], checkpoint['ema_' + k] = (avg, checkpoint[k]) if self._ema_active else (checkpoint[k], avg)
        if self._ema:
            checkpoint['ema_decay'] = float(self.opt.ema_decay)
        checkpoint.update({k: o.state_dict() for k, o in self._optimizers().items()})
        torch.save(checkpoint, chk_path)

    def load(self, chk_path, use_ema=False):
        """use_ema: the networks themselves take the checkpoint's averaged weights (`ema_<net>`; KeyError naming the missing
        key for a checkpoint without them), on any model.  A model that keeps averages restores them from the checkpoint, or,
        from one without them, starts them at the loaded parameters."""
        self._live_only("load")
        checkpoint = torch.load(chk_path, map_location=self._dev())
        if use_ema:
            for k in self.EMA_NETS:
                if 'ema_' + k not in checkpoint:
                    raise KeyError("checkpoint %s holds no averaged weights: key 'ema_%s' is missing (written by a run "
                                   "without --ema_decay?)" % (chk_path, k))
        for k, n in self._net_dict().items():
            n.load_state_dict(checkpoint['ema_' + k if use_ema and k in self.EMA_NETS else k])
            mark_dirty(n)
        for k, o in self._optimizers().items():
            o.load_state_dict(checkpoint[k])
        restart = []
        for k, f in self._ema:
            sd = None if use_ema else checkpoint.get('ema_' + k)
            if sd is None:
                f.ema.copy_(f.p)
                restart.append(k)
                continue
            for (name, p), o in zip(f.net.named_parameters(), f.offs):
                f.ema[o:o + p.numel()].copy_(sd[name].reshape(-1))
        if restart and not use_ema:
            print("load: %s holds no averaged weights for %s; the averages start at the loaded parameters"
                  % (chk_path, ", ".join(restart)))


def _as2d(t):
    """public-API tensors (NCHW / (N,C)) -> (rows, Cp) C16 view for the loss kernels"""
    if t.dim() == 4:
        return ops.ToNHWC.apply(t).reshape(-1, cpad(t.shape[1]))
    return t.reshape(t.shape[0], -1)


def discriminate(net, crit, fake, real):
    """model.py:327-334 (public-API form)"""
    pred_fake = net(fake)
    loss_fake = crit(pred_fake, False)
    pred_true = net(real)
    loss_true = crit(pred_true, True)
    return loss_fake, loss_true, pred_fake, pred_true


class AugmentedCycleGAN(_Base):
    """Augmented cycle gan — model.py:337-794"""

    def __init__(self, opt, testing=False):
        self._exchanges = {}
        self.old_lr = opt.lr
        opt.use_sigmoid = opt.no_lsgan
        self.opt = opt
        nb = _n_blocks(opt)
        self.netG_A_B = networks.define_stochastic_G(nlatent=opt.nlatent, input_nc=opt.input_nc, output_nc=opt.output_nc,
                                                     ngf=opt.ngf, which_model_netG=opt.which_model_netG, norm=opt.norm,
                                                     use_dropout=opt.use_dropout, gpu_ids=opt.gpu_ids, n_blocks=nb)
        self.netG_B_A = networks.define_G(input_nc=opt.output_nc, output_nc=opt.input_nc, ngf=opt.ngf,
                                          which_model_netG=opt.which_model_netG, norm=opt.norm,
                                          use_dropout=opt.use_dropout, gpu_ids=opt.gpu_ids, n_blocks=nb)
        enc_input_nc = opt.output_nc
        if opt.enc_A_B:
            enc_input_nc += opt.input_nc
        self.netE_B = networks.define_E(nlatent=opt.nlatent, input_nc=enc_input_nc, nef=opt.nef, norm='batch',
                                        gpu_ids=opt.gpu_ids)
        self.netD_A = networks.define_D_A(input_nc=opt.input_nc, ndf=32, which_model_netD=opt.which_model_netD,
                                          norm=opt.norm, use_sigmoid=opt.use_sigmoid, gpu_ids=opt.gpu_ids)
        self.netD_B = networks.define_D_B(input_nc=opt.output_nc, ndf=opt.ndf, which_model_netD=opt.which_model_netD,
                                          norm=opt.norm, use_sigmoid=opt.use_sigmoid, gpu_ids=opt.gpu_ids)
        self.netD_z_B = networks.define_LAT_D(nlatent=opt.nlatent, ndf=opt.ndf, use_sigmoid=opt.use_sigmoid,
                                              gpu_ids=opt.gpu_ids)
        self._build_optimizers()
        # --no_lsgan: the reference binds its (broken) BCE branch here; the float-target fix
        self.criterionGAN = criterion_GAN_bce if opt.use_sigmoid else functools.partial(criterion_GAN, use_sigmoid=False)
        self.criterionCycle = lambda a, b: ops.L1.apply(_as2d(a), _as2d(b), a.shape[1])
        if not testing:
            with open("%s/nets.txt" % opt.expr_dir, 'w') as nets_f:
                for n in (self.netG_A_B, self.netG_B_A, self.netD_A, self.netD_B, self.netD_z_B, self.netE_B):
                    networks.print_network(n, nets_f)                                           # model.py:393-400

    def _nets(self):
        return [self.netG_A_B, self.netG_B_A, self.netE_B, self.netD_A, self.netD_B, self.netD_z_B]

    def _build_optimizers(self):
        o = self.opt
        acg_dist.broadcast_params_(self._nets())
        self.f_G_A_B, self.f_G_B_A, self.f_E_B = FlatNet(self.netG_A_B), FlatNet(self.netG_B_A), FlatNet(self.netE_B)
        self.f_D_A, self.f_D_B, self.f_D_z_B = FlatNet(self.netD_A), FlatNet(self.netD_B), FlatNet(self.netD_z_B)
        b = (o.beta1, 0.999)
        self.optimizer_G_A = FusedAdam([self.f_G_B_A], o.lr, b)                                 # model.py:379-380
        self.optimizer_G_B = FusedAdam([self.f_G_A_B, self.f_E_B], o.lr, b)                     # model.py:381-383
        self.optimizer_D_A = FusedAdam([self.f_D_A], o.lr / 5., b)                              # model.py:384-385
        self.optimizer_D_B = FusedAdam([self.f_D_B, self.f_D_z_B], o.lr / 5., b)                # model.py:386-389
        self._setup_ema()

    EMA_NETS = ('netG_A_B', 'netG_B_A', 'netE_B')    # the networks of optimizer_G_A and optimizer_G_B

    def _encode(self, a_or_fake_a, b):
        """E_B on cat((A-side, B-side), 1) (A first: model.py:410, 472) -> (mu, logvar) (N, cpad(nl))"""
        o = self.opt
        x = ops.Concat.apply(a_or_fake_a, b, o.input_nc, o.output_nc) if o.enc_A_B else b
        return self.netE_B.forward_nhwc(x)

    def train_instance(self, real_A, real_B, prior_z_B):
        self._live_only("train_instance")
        if self._step_graph is not None and not acg_dist.exchange_on():
            return self._step_graph(real_A, real_B, prior_z_B)
        with _in_train_step():
            return self._train_instance(real_A, real_B, prior_z_B)

    def _train_instance(self, real_A, real_B, prior_z_B):
        o = self.opt
        nA, nB, nl = o.input_nc, o.output_nc, o.nlatent
        flats_D = [self.f_D_A, self.f_D_B, self.f_D_z_B]
        for f in flats_D + [self.f_G_A_B, self.f_G_B_A, self.f_E_B]:
            f.check()
        A, B, z = ops.ToNHWC.apply(real_A, True), ops.ToNHWC.apply(real_B, True), as_latent(prior_z_B)
        bs = z.shape[0]

        fake_B = self.netG_A_B.forward_nhwc(A, z)                                               # model.py:404
        fake_A = self.netG_B_A.forward_nhwc(B)                                                  # model.py:407
        mu_rB, lv_rB = self._encode(fake_A, B)                                                  # model.py:409-413
        if o.stoch_enc:
            post_z = gauss_reparametrize(mu_rB[:, :nl], lv_rB[:, :nl]).view(bs, nl)             # model.py:416
        else:
            post_z = mu_rB                                                                      # model.py:418
            lv_rB = lv_rB * 0.0                                                                 # model.py:419

        # ---- D phase (model.py:423-452)
        p_fA = self.netD_A.forward_nhwc(fake_A.detach()); l_fA = self._gan_loss(p_fA, False)
        p_tA = self.netD_A.forward_nhwc(A); l_tA = self._gan_loss(p_tA, True)
        p_fB = self.netD_B.forward_nhwc(fake_B.detach()); l_fB = self._gan_loss(p_fB, False)
        p_tB = self.netD_B.forward_nhwc(B); l_tB = self._gan_loss(p_tB, True)
        l_pz = self._gan_loss(self.netD_z_B.forward_dense(post_z.detach()), False)
        l_rz = self._gan_loss(self.netD_z_B.forward_dense(z), True)
        loss_D_A, loss_D_B, loss_D_z_B = 0.5 * (l_fA + l_tA), 0.5 * (l_fB + l_tB), 0.5 * (l_pz + l_rz)
        loss_D = loss_D_A + loss_D_B
        z_gan = bool(o.z_gan and not o.stoch_enc)
        if z_gan:
            loss_D = loss_D + loss_D_z_B
        self.optimizer_D_A.zero_grad(); self.optimizer_D_B.zero_grad()
        # completion order of the D backward = reverse build order: D_z_B, D_B, D_A (without the latent GAN term D_z_B
        # receives no gradient at all, model.py:438-439, and goes last)
        order_D = [self.f_D_z_B, self.f_D_B, self.f_D_A] if z_gan else [self.f_D_B, self.f_D_A, self.f_D_z_B]
        ex_D = self._backward(loss_D, "aug.D", order_D)
        m_tA, m_tB = ops.mean_valid(p_tA, 1), ops.mean_valid(p_tB, 1)

        # ---- G phase (model.py:457-515).  The cycle / encoder forwards (model.py:467-494) do not depend on the
        # discriminators: they are enqueued first and run while the D gradients are being all-reduced ...
        rec_A = self.netG_B_A.forward_nhwc(fake_B); loss_cycle_A = ops.L1.apply(rec_A, A, nA)
        mu_fB, lv_fB = self._encode(A, fake_B)                                                  # model.py:471-475
        if o.stoch_enc:
            lp = log_prob_gaussian(z, mu_fB[:, :nl], lv_fB[:, :nl])
            loss_cycle_z_B = -1.0 * lp.mean(1).mean(0)                                          # model.py:480-484
        else:
            loss_cycle_z_B = ops.L1.apply(mu_fB, _pad_cols(z, mu_fB.shape[1]), nl)              # model.py:486-487
        rec_B = self.netG_A_B.forward_nhwc(fake_A, post_z); loss_cycle_B = ops.L1.apply(rec_B, B, nB)
        kld_z_B = kld_std_guss(mu_rB[:, :nl], lv_rB[:, :nl]).mean(0)                            # model.py:490
        # ... the discriminator forwards need the UPDATED discriminators (model.py:455-457)
        self._wait(ex_D, self.f_D_A)
        (ss_D_A,) = self.optimizer_D_A.clip_and_step(o.max_gnorm)
        self._wait(ex_D, self.f_D_B, self.f_D_z_B)
        ss_D_B, ss_D_z = self.optimizer_D_B.clip_and_step(o.max_gnorm)
        ss_D_A, ss_D_B, ss_D_z = ss_D_A.clone(), ss_D_B.clone(), ss_D_z.clone()
        for f in flats_D:                                   # D weight gradients are not needed in the G phase
            f.set_requires_grad(False)
        try:
            p_fA = self.netD_A.forward_nhwc(fake_A); loss_G_A = self._gan_loss(p_fA, True)
            p_fB = self.netD_B.forward_nhwc(fake_B); loss_G_B = self._gan_loss(p_fB, True)
            loss_G_z_B = self._gan_loss(self.netD_z_B.forward_dense(post_z), True)
            loss_G = loss_G_A + loss_G_B + loss_cycle_A * o.lambda_A + loss_cycle_B * o.lambda_B \
                + loss_cycle_z_B * o.lambda_z_B
            if o.stoch_enc:
                loss_G = loss_G + kld_z_B * o.lambda_z_B
            if z_gan:
                loss_G = loss_G + loss_G_z_B
            loss_G, opt_sums, opt_names = losses.add_terms(self, losses.UNPAIRED, loss_G, A, B, z,
                                                           fake=(fake_A, fake_B), rec=(rec_A, rec_B))
            self.optimizer_G_A.zero_grad(); self.optimizer_G_B.zero_grad()
            mu_v, lv_v = mu_rB.detach()[:, :nl], lv_rB.detach()[:, :nl]
            sums = [loss_D_A, loss_G_A, loss_cycle_A, loss_cycle_z_B, kld_z_B, loss_D_B, loss_G_B, loss_cycle_B,
                    loss_D_z_B, m_tA, ops.mean_valid(p_fA, 1), m_tB, ops.mean_valid(p_fB, 1)] + opt_sums
            mins, maxs = [mu_v.min(), lv_v.min()], [mu_v.max(), lv_v.max()]
            # completion order of the G backward: E_B (its first call is the last of the three first-pass networks to have
            # been built), then G_B_A, then G_A_B — which therefore carries the scalar tail
            ex_G = self._backward(loss_G, "aug.G", [self.f_E_B, self.f_G_B_A, self.f_G_A_B],
                                  tail=(self.f_G_A_B, sums, mins + maxs))
        finally:
            for f in flats_D:
                f.set_requires_grad(True)
        self._wait(ex_G, self.f_G_B_A)
        (ss_G_B_A,) = self.optimizer_G_A.clip_and_step(o.max_gnorm)
        self._wait(ex_G, self.f_G_A_B, self.f_E_B)
        ss_G_A_B, ss_E = self.optimizer_G_B.clip_and_step(o.max_gnorm)

        n_loss = len(sums)
        names = ['D_A', 'G_A', 'Cyc_A', 'Cyc_z_B', 'KLD_z_B', 'D_B', 'G_B', 'Cyc_B', 'D_z_B',
                 'P_t_A', 'P_f_A', 'P_t_B', 'P_f_B'] + opt_names + [
                 'gnorm_G_A_B', 'gnorm_G_B_A', 'gnorm_E_B', 'gnorm_D_B', 'gnorm_D_z_B', 'gnorm_D_A',
                 'mu_min', 'logvar_min', 'mu_max', 'logvar_max']
        vals = self._scalars(ex_G, self.f_G_A_B, names, sums, mins, maxs,
                             local=[ss_G_A_B, ss_G_B_A, ss_E, ss_D_B, ss_D_z, ss_D_A])
        visuals = OrderedDict([('real_A', real_A.detach()), ('fake_B', self._nchw(fake_B, nB)),
                               ('rec_A', self._nchw(rec_A, nA)), ('real_B', real_B.detach()),
                               ('fake_A', self._nchw(fake_A, nA)), ('rec_B', self._nchw(rec_B, nB))])

        def finish(vals):
            losses = OrderedDict((k, vals[k]) for k in names[:n_loss])                          # model.py:518-523
            if o.monitor_gnorm:
                gnorms = OrderedDict((k, math.sqrt(max(vals[k], 0.0))) for k in names[n_loss:n_loss + 6])   # model.py:527-533
                for k in ('mu_min', 'mu_max', 'logvar_min', 'logvar_max'):
                    gnorms[k] = vals[k]
                return losses, visuals, gnorms
            return losses, visuals
        return self._report(vals, finish)

    def supervised_train_instance(self, real_A, real_B, prior_z_B):
        """model.py:541-604 (paired step; off by default, --supervised)"""
        self._live_only("supervised_train_instance")
        if self._sup_step_graph is not None and not acg_dist.exchange_on():
            return self._sup_step_graph(real_A, real_B, prior_z_B)
        with _in_train_step():
            return self._supervised_train_instance(real_A, real_B, prior_z_B)

    def _supervised_train_instance(self, real_A, real_B, prior_z_B):
        o = self.opt
        nA, nB, nl = o.input_nc, o.output_nc, o.nlatent
        A, B, z = ops.ToNHWC.apply(real_A, True), ops.ToNHWC.apply(real_B, True), as_latent(prior_z_B)
        bs = z.shape[0]
        mu, logvar = self._encode(A, B)
        if o.stoch_enc:
            post_z = gauss_reparametrize(mu[:, :nl], logvar[:, :nl]).view(bs, nl)
        else:
            post_z = mu
            logvar = logvar * 0.0
        l_pz = self._gan_loss(self.netD_z_B.forward_dense(post_z.detach()), False)
        l_rz = self._gan_loss(self.netD_z_B.forward_dense(z), True)
        loss_D_z_B = 0.5 * (l_pz + l_rz)
        self.optimizer_D_B.zero_grad()
        ex_D = self._backward(loss_D_z_B, "sup.D", [self.f_D_z_B, self.f_D_B])
        self._wait(ex_D, self.f_D_B, self.f_D_z_B)
        _, ss_D_z = self.optimizer_D_B.clip_and_step(o.max_gnorm)
        ss_D_z = ss_D_z.clone()
        self.f_D_z_B.set_requires_grad(False)
        try:
            pred_B = self.netG_A_B.forward_nhwc(A, post_z)
            pred_A = self.netG_B_A.forward_nhwc(B)
            loss_sup_A = ops.L1.apply(pred_A, A, nA)
            loss_sup_B = ops.L1.apply(pred_B, B, nB)
            loss_G_z_B = self._gan_loss(self.netD_z_B.forward_dense(post_z), True)
            kld_z_B = kld_std_guss(mu[:, :nl], logvar[:, :nl]).mean(0)
            loss_G = loss_sup_A * o.lambda_sup_A + loss_sup_B * o.lambda_sup_B
            if o.stoch_enc:
                loss_G = loss_G + kld_z_B * o.lambda_z_B
            if o.z_gan and not o.stoch_enc:
                loss_G = loss_G + loss_G_z_B
            loss_G, opt_sums, opt_names = losses.add_terms(self, losses.PAIRED, loss_G, A, B, z, pred=(pred_A, pred_B))
            self.optimizer_G_A.zero_grad(); self.optimizer_G_B.zero_grad()
            sums = [loss_sup_A, loss_sup_B, kld_z_B, loss_D_z_B] + opt_sums
            # the order in which the networks' gradients complete: G_B_A (its only pass hangs on nothing else), G_A_B, then
            # the encoder behind post_z.  With the CRPS term G_A_B's member pass is built last and runs backward first, but
            # G_A_B is complete only after its first pass, which still finishes after G_B_A's and before the encoder's
            ex_G = self._backward(loss_G, "sup.G", [self.f_G_B_A, self.f_G_A_B, self.f_E_B], tail=(self.f_E_B, sums))
        finally:
            self.f_D_z_B.set_requires_grad(True)
        self._wait(ex_G, self.f_G_B_A)
        (ss_G_B_A,) = self.optimizer_G_A.clip_and_step(o.max_gnorm)
        self._wait(ex_G, self.f_G_A_B, self.f_E_B)
        ss_G_A_B, ss_E = self.optimizer_G_B.clip_and_step(o.max_gnorm)
        n_loss = len(sums)
        names = ['S_A', 'S_B', 'KLD_z_B', 'D_z_B'] + opt_names + ['gnorm_G_A_B', 'gnorm_G_B_A', 'gnorm_E_B', 'gnorm_D_z_B']
        vals = self._scalars(ex_G, self.f_E_B, names, sums, local=[ss_G_A_B, ss_G_B_A, ss_E, ss_D_z])

        def finish(vals):
            for k in names[n_loss:]:
                vals[k] = math.sqrt(max(vals[k], 0.0))
            return vals                                                                         # model.py:596-604
        return self._report(vals, finish)

    # ---- hooks of the shared forward-only helpers (_Base) + the encoder-specific ones (model.py:606-733) ----
    _noise_before_code = True

    def _z(self, z):
        return z

    def _enc_public(self, a, b):
        x = torch.cat((a, b), 1) if self.opt.enc_A_B else b
        return self.netE_B.forward(x)

    def _post_z(self, mu, logvar):
        if self.opt.stoch_enc:
            return gauss_reparametrize(mu, logvar)
        return mu.reshape(mu.size(0), mu.size(1), 1, 1)

    def _cycle_code(self, fake_A, real_B, prior_z_B):
        """the code the B -> A -> B cycle is closed with: the encoder's posterior for (fake_A, real_B)"""
        return self._post_z(*self._enc_public(fake_A, real_B))

    def predict_enc_params(self, real_A, real_B):
        """model.py:653-662"""
        mu, logvar = self._enc_public(real_A, real_B)
        return (mu, logvar) if self.opt.stoch_enc else (mu,)

    def generate_multi_cycle(self, real_B, steps, from_prior=True):
        """model.py:664-685: alternate B -> A -> B `steps` times, re-drawing (or re-encoding) the code every round"""
        images, B = [real_B.data], real_B
        for _ in range(steps):
            A = self.predict_A(B)
            code = self._draw_prior(real_B) if from_prior else self._cycle_code(A, B, None)
            B = self.netG_A_B.forward(A, code)
            images += [A.data, B.data]
        return images

    def inference_multi(self, real_A, real_B):
        """model.py:710-733: every A against the posterior code of every B — (|A| * |B|) images, A-major"""
        codes = self._cycle_code(self.predict_A(real_B) if self.opt.enc_A_B else real_B, real_B, None)
        return self.netG_A_B.forward(_each_n_times(real_A, real_B.size(0)), codes.data.repeat(real_A.size(0), 1, 1, 1))

    def _optimizers(self):
        return OrderedDict([('optimizer_D_A', self.optimizer_D_A), ('optimizer_G_A', self.optimizer_G_A),
                            ('optimizer_D_B', self.optimizer_D_B), ('optimizer_G_B', self.optimizer_G_B)])

    def _net_dict(self):
        return OrderedDict([('netG_A_B', self.netG_A_B), ('netG_B_A', self.netG_B_A), ('netD_A', self.netD_A),
                            ('netD_B', self.netD_B), ('netD_z_B', self.netD_z_B), ('netE_B', self.netE_B)])

    update_learning_rate = StochCycleGAN.update_learning_rate                                    # model.py:735-748
    save = StochCycleGAN.save                                                                    # model.py:750-764
    load = StochCycleGAN.load                                                                    # model.py:766-778


# north-star alias (BASELINE.json names the class AugmentedCycleGAN_Model)
AugmentedCycleGAN_Model = AugmentedCycleGAN
