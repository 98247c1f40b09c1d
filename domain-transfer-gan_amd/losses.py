"""The optional losses of the training steps: one record per family, in the fixed order spec, marg, ssim, crps, fss.

Everything that must know which families exist reads FAMILIES: the three step methods of model.py (add_terms: the
terms, their scalars and the scalars' names), StepGraph._key (key_options: what a captured step bakes in),
TrainOptions.parse (the four refusals every family shares) and train.py (is the fss loss on).  A new family is one
record here plus its kernel behind an ops.py function."""
from collections import namedtuple

import torch

from . import ops

UNPAIRED, PAIRED = 'unpaired', 'paired'     # the steps: _train_instance of either model, _supervised_train_instance


class Family(namedtuple('Family', 'stem sides reads steps grid paired_only negative_ok term')):
    """stem, sides: the weights are --lambda_<stem>_<side> for every side in `sides` ('AB', or 'B' alone).
    reads: the other options the term reads (with the weights: what a captured step bakes in of this family).
    steps: {step: (operands, names)} - the steps that carry the term, which of the tensors the step hands to add_terms
        it takes there (a keyword of add_terms naming an (A side, B side) pair, or None) and the scalars it reports.
    grid: (lo, hi, power of two only, the phrase of the refusal) - the --grid_size a positive weight needs.
    paired_only: a term of the paired step alone (a positive weight needs --supervised and a model with a paired step).
    negative_ok: the parser lets a negative weight pass (it reads as off).
    term(model, family, A, B, z, x_A, x_B) -> (scalar, scalar, weighted term for loss_G), called only when a weight is
        positive."""

    def options(self):
        return ['lambda_%s_%s' % (self.stem, s) for s in self.sides]

    def flags(self):
        return ' / '.join('--' + o for o in self.options())

    def weights(self, opt):
        """the weights in the order of `sides`; 0 for options written before the family existed (opt.pkl)"""
        return tuple(float(getattr(opt, o, 0.0) or 0.0) for o in self.options())

    def on(self, opt):
        return any(w > 0 for w in self.weights(opt))


def _two_sided(loss):
    """the term of a family that is `ops.<loss>(x, real, C, "nhwc")` on either side: model._optional_terms"""
    def term(model, fam, A, B, z, x_A, x_B):
        return model._optional_terms(getattr(ops, loss), fam.weights(model.opt), x_A, A, x_B, B)
    return term


def _crps_term(model, fam, A, B, z, x_A, x_B):
    """S_crps_B, S_pair_B: the almost fair CRPS of Me = min(crps_members, batch) translations of every paired input
    against its B, the members' mean pair distance, the weighted term for loss_G.  The members are one more pass of G_A_B,
    in the step's train state, over every input repeated Me times in a row; member m of input n is coded with
    z[(n + m) % batch]: prior draws the step already has, independent of the inputs and distinct per input, so no new
    random number enters the step and a captured step replays it.  Neither the encoder nor G_B_A is on the term's path."""
    from .model import ensemble_chunk
    o = model.opt
    (lam,) = fam.weights(o)
    bs = z.shape[0]
    members = int(getattr(o, 'crps_members', 4))
    if not 2 <= members <= ops.CRPS_MAX_M:
        raise ValueError("crps_members must lie in 2..%d (got %d)" % (ops.CRPS_MAX_M, members))
    Me = min(members, bs)
    most = ensemble_chunk(o.ngf, A.shape[1], A.shape[2])
    if bs * Me > most:
        raise ValueError("lambda_crps_B: %d inputs x %d members are more than the %d images one generator pass holds at "
                         "%d x %d with ngf %d" % (bs, Me, most, A.shape[1], A.shape[2], o.ngf))
    inputs = A.unsqueeze(1).expand((bs, Me) + tuple(A.shape[1:])).reshape((bs * Me,) + tuple(A.shape[1:]))
    codes = torch.stack([torch.roll(z, -m, 0) for m in range(Me)], 1).reshape(bs * Me, z.shape[1])
    fakes = model.netG_A_B.forward_nhwc(inputs, codes)
    loss, _, pair = ops.crps_loss(fakes, B, o.output_nc, "nhwc", "nhwc", Me,
                                  alpha=float(getattr(o, 'crps_alpha', 0.95)), parts=True)
    return loss, pair, loss * lam


def _fss_term(model, fam, A, B, z, pred_A, pred_B):
    """S_fss_A, S_fss_B (ops.fss_loss: 1 - the fractions skill score of soft threshold exceedances, pooled over the
    batch), as model._optional_terms gives them.  Each side has its own thresholds, opt.fss_loss_thr_A / _B ((C, T)
    nested lists, the climatology train.py resolves at start), uploaded once; the windows (fss_loss_windows) and the
    temperature (fss_tau) are shared.  Under the data-parallel exchange every rank pools its own batch, as the marginal
    loss does, and the reported scalars are the ranks' average."""
    o = model.opt
    windows, tau = tuple(getattr(o, 'fss_loss_windows', (3, 9, 17))), float(getattr(o, 'fss_tau', 0.05))

    def side(name):
        thr = getattr(o, 'fss_loss_thr_' + name, None)
        if thr is None:
            raise ValueError("lambda_fss_A / lambda_fss_B: the options hold no thresholds: fss_loss_thr_A and fss_loss_thr_B "
                             "must be (C, T) nested lists (train.py resolves them from fss_loss_quantiles / "
                             "fss_loss_thresholds)")
        cache = model.__dict__.setdefault('_fss_thr_dev', {})
        key = (name, hashable(thr))
        if key not in cache:                                   # once; device fills, no host copy: a capture can record them
            flat = [float(v) for row in thr for v in row]
            table = torch.empty(len(flat), dtype=torch.float32, device=pred_A.device)
            for i, v in enumerate(flat):
                table[i].fill_(v)
            cache[key] = table.reshape(len(thr), -1)
        return lambda fake, real, C, layout: ops.fss_loss(fake, real, C, layout, cache[key], windows, tau)
    sides = side('A'), side('B')
    return model._optional_terms(sides, fam.weights(o), pred_A, A, pred_B, B)


_TO_1024 = "fields of up to 1024 x 1024"

FAMILIES = (
    # batch-mean radial spectra of the fakes against the real batches.  A negative --lambda_spec_* has never been refused
    # (it reads as off); the later families refuse theirs.  Kept as it is: commands accepted so far stay accepted.
    Family('spec', 'AB', (), {UNPAIRED: ('fake', ['Spec_A', 'Spec_B'])},
           (16, 1024, True, "the spectral loss needs fields of S x S with S a power of two in 16..1024"),
           False, True, _two_sided('spectral_loss')),
    # the distance of the two batches' mean quantile functions, fakes against the real batches
    Family('marg', 'AB', (), {UNPAIRED: ('fake', ['Marg_A', 'Marg_B'])},
           (1, 1024, False, "the marginal loss sorts " + _TO_1024), False, False, _two_sided('marginal_loss')),
    # 1 - the mean structural similarity of the pairs a step has: the CYCLE reconstructions against their real batches in
    # an unpaired step, the predictions against their paired fields in the paired one
    Family('ssim', 'AB', (), {UNPAIRED: ('rec', ['Ssim_A', 'Ssim_B']), PAIRED: ('pred', ['S_ssim_A', 'S_ssim_B'])},
           (11, 1024, False, "the structural similarity slides an 11 x 11 window over " + _TO_1024),
           False, False, _two_sided('ssim_loss')),
    # B only: B -> A is deterministic, an ensemble of one, whose CRPS is the L1 term the paired step already has
    Family('crps', 'B', ('crps_members', 'crps_alpha'), {PAIRED: (None, ['S_crps_B', 'S_pair_B'])},
           (1, 1024, False, "the CRPS loss takes " + _TO_1024), True, False, _crps_term),
    Family('fss', 'AB', ('fss_tau', 'fss_loss_windows', 'fss_loss_thr_A', 'fss_loss_thr_B'),
           {PAIRED: ('pred', ['S_fss_A', 'S_fss_B'])},
           (1, 1024, False, "the fss loss takes " + _TO_1024), True, False, _fss_term),
)
BY_STEM = dict((f.stem, f) for f in FAMILIES)


def hashable(v):
    """an option's value as a key: lists (the windows and the nested threshold tables of the fss loss) become tuples"""
    return tuple(hashable(x) for x in v) if isinstance(v, (list, tuple)) else v


def key_options():
    """every option of every family, weights first: what a captured step bakes in besides the options of no family"""
    return [o for f in FAMILIES for o in f.options() + list(f.reads)]


def active(opt, step):
    return [f for f in FAMILIES if step in f.steps and f.on(opt)]


def names(opt, step):
    """the names of the optional loss scalars `step` appends to its fixed ones, in the order of its sums"""
    return [n for f in active(opt, step) for n in f.steps[step][1]]


def add_terms(model, step, loss_G, A, B, z, **outputs):
    """The optional terms of one step, formed and added to loss_G in the order of FAMILIES (unpaired: spec, marg, ssim;
    paired: ssim, crps, fss).  A, B, z: the step's internal NHWC batches and its prior draws; outputs: the (A side, B side)
    pairs the records name (fake=, rec= in an unpaired step, pred= in the paired one).  Returns (loss_G with every
    weighted term added, the scalars to append to the step's sums, their names).  With every weight 0 (the default) no
    tensor is touched and no launch is issued."""
    sums = []
    for fam in active(model.opt, step):
        operands = fam.steps[step][0]
        x_A, x_B = outputs[operands] if operands else (None, None)
        t0, t1, add = fam.term(model, fam, A, B, z, x_A, x_B)
        loss_G = loss_G + add
        sums += [t0, t1]
    return loss_G, sums, names(model.opt, step)
