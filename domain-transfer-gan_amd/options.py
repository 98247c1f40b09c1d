"""Command-line options — Py3 counterpart of /root/reference/augmented_cyclegan/options.py (which is Python 2:
`import cPickle`, options.py:4).  Same flags, defaults, `opt.txt` format, `opt.pkl`, sub-directory creation
(options.py:7-12, 20-131).  Additions (not in the reference): --n_blocks, --precision, --synthetic, --dist,
--step_graph, --defer_scalars, --lambda_spec_A, --lambda_spec_B, --ema_decay, --ema_eval,
--lambda_marg_A, --lambda_marg_B, --native_res, --window_flip, --lambda_fss_A, --lambda_fss_B (with --fss_loss_quantiles,
--fss_loss_thresholds, --fss_loss_windows, --fss_tau)."""
import argparse
import os
import pickle

import torch

from .losses import BY_STEM, FAMILIES


def create_sub_dirs(opt, sub_dirs):
    """options.py:7-12"""
    for sub_dir in sub_dirs:
        dir_path = os.path.join(opt.expr_dir, sub_dir)
        os.makedirs(dir_path, exist_ok=True)
        setattr(opt, sub_dir, dir_path)


# flag table: (name, kind, default, help).  kind is a type, a ("choice", type, values) tuple, or "flag".
# Values and order follow options.py:20-85 of the reference; the last group is new here.
_T = [
    ("dataroot", str, None, "path to data (trainA/B.npz, testA/B.npz)"),
    ("checkpoints_dir", str, "./checkpoints/", "models are saved here"),
    # data
    ("input_nc", int, 3, "# of input image channels"),
    ("output_nc", int, 3, "# of output image channels"),
    ("grid_size", int, 256, "resolution of input/output grids"),
    ("numpy_data", ("choice", int, [0, 1]), 1, "use numpy data"),
    # experiment
    ("seed", int, None, "manual seed"),
    ("model", ("choice", str, ["cycle_gan", "stoch_cycle_gan", "aug_cycle_gan"]), "aug_cycle_gan", "which model to train"),
    ("gpu_ids", str, "0", 'gpu ids: e.g. 0  0,1,2 (only "on the GPU" matters here; -1 is rejected later: no CPU path)'),
    # supervised training
    ("supervised", "flag", False, "also run the paired step"),
    ("sup_frac", float, 0.1, "fraction of training data for supervised training"),
    ("lambda_sup_A", float, 0.1, "weight for supervised loss (B -> A)"),
    ("lambda_sup_B", float, 0.1, "weight for supervised loss (A -> B)"),
    # training
    ("batchSize", int, 32, "input batch size"),
    ("continue_train", "flag", False, "reload <expr_dir>/<which_epoch> before training"),
    ("which_epoch", str, "latest", "checkpoint name to resume from"),
    ("epoch_count", int, 1, "the starting epoch count"),
    ("niter", int, 25, "# of epochs at starting learning rate"),
    ("niter_decay", int, 25, "# of epochs to linearly decay learning rate to zero"),
    ("beta1", float, 0.5, "momentum term of adam"),
    ("lr", float, 0.0002, "initial learning rate for adam"),
    # model
    ("ngf", int, 32, "# of gen filters in first conv layer"),
    ("nef", int, 32, "# of encoder filters in first conv layer"),
    ("ndf", int, 64, "# of discrim filters in first conv layer"),
    ("nlatent", int, 16, "# of latent code dimensions"),
    ("which_model_netD", str, "basic", "(accepted, unused — as in the reference)"),
    ("which_model_netG", str, "resnet", "(accepted, unused — as in the reference)"),
    ("norm", str, "instance", "instance or batch normalization"),
    ("use_dropout", "flag", False, "use dropout for the generator"),
    ("max_gnorm", float, 500., "max grad norm to which it will be clipped"),
    ("stoch_enc", "flag", False, "use a stochastic encoder"),
    ("z_gan", ("choice", int, [0, 1]), 1, "use a GAN on z_B"),
    ("enc_A_B", ("choice", int, [0, 1]), 1, "encoder of z_B conditioned on both A and B"),
    ("no_lsgan", "flag", False, "vanilla GAN: sigmoid discriminator heads and binary cross-entropy with a float target (the reference's Long target fails)"),
    ("lambda_A", float, 1.0, "weight for cycle loss (A -> B -> A)"),
    ("lambda_B", float, 1.0, "weight for cycle loss (B -> A -> B)"),
    ("lambda_z_B", float, 0.025, "weight for the latent cycle loss"),
    # monitoring
    ("monitor_gnorm", bool, True, "monitor grad norms (type=bool as in options.py:77: any string is True)"),
    ("display_freq", int, 5000, "frequency of PNG dumps"),
    ("print_freq", int, 100, "frequency of log lines"),
    ("save_epoch_freq", int, 5, "frequency of saving checkpoints at the end of epochs"),
    ("num_multi", int, 10, "the number of z_B used to generate different B"),
    ("eval_A_freq", int, 1, "frequency of evaluating on A"),
    ("eval_B_freq", int, 1, "frequency of evaluating on B"),
    # additions of this implementation
    ("n_blocks", int, 3, "residual blocks per generator (the reference builds 3)"),
    ("precision", ("choice", str, ["bf16x3", "f32"]), "bf16x3",
     "conv arithmetic on the matrix cores: bf16x3 (default; split-bf16 products, inside the 1e-3 parity bar — what bench.py "
     "and the parity tests run), f32 (exact products, 2.4x slower)"),
    ("synthetic", int, 0, "use N synthetic U(-1,1) samples per split instead of --dataroot"),
    ("sync_bn", "flag", False, "data parallel: BatchNorm (E_B, D_z_B) statistics across all ranks"),
    ("step_graph", "flag", False, "replay the training step (and, with --supervised, the paired step from a second graph) as "
                                  "one captured HIP graph (launch-bound sizes: small images / batches; single GPU: under the "
                                  "data-parallel exchange both steps run eagerly)"),
    ("defer_scalars", "flag", False, "with --step_graph: a replayed step hands its losses back later, read only on --print_freq "
                                     "/ --display_freq steps, so the host enqueues the next step while this one runs (at most "
                                     "2 in flight); the logged numbers are those of --step_graph alone"),
    ("eval_steps", int, 50, "variational-bound steps per epoch (train.py:285 uses 50)"),
    ("lambda_spec_A", float, 0.0, "weight of the spectral loss on fake_A against the real A: the squared log distance of the "
                                  "batch-mean radially averaged power spectra (ops.spectral_loss); 0: off; needs --grid_size "
                                  "a power of two in 16..1024"),
    ("lambda_spec_B", float, 0.0, "the same on fake_B against the real B"),
    ("ema_decay", float, 0.0, "keep an exponential moving average of the generator-side weights (G_A_B, G_B_A, E_B) behind every "
                              "optimiser step, with this decay (e.g. 0.999; warm-up min(decay, (1 + t) / (10 + t))); saved as "
                              "ema_<net> next to the live weights; 0: off; inside [0, 1)"),
    ("ema_eval", ("choice", int, [0, 1]), 1, "with --ema_decay: the per-epoch evaluation and the dev-set visualisations score "
                                             "the averaged weights (1) or the live ones (0)"),
    ("lambda_marg_A", float, 0.0, "weight of the marginal loss on fake_A against the real A: the squared 2-Wasserstein distance "
                                  "of the two batches' mean quantile functions, per channel (ops.marginal_loss: every field is "
                                  "sorted); 0: off; needs --grid_size up to 1024"),
    ("lambda_marg_B", float, 0.0, "the same on fake_B against the real B"),
    ("lambda_ssim_A", float, 0.0, "weight of the structural-similarity loss 1 - SSIM (ops.ssim_loss: 11 x 11 Gaussian window, "
                                  "sigma 1.5, data range 2) on the cycle reconstruction rec_A against the real A, and with "
                                  "--supervised on the paired prediction of A; 0: off; needs 11 <= --grid_size <= 1024"),
    ("lambda_ssim_B", float, 0.0, "the same on rec_B (and the paired prediction of B) against the real B"),
    ("lambda_crps_B", float, 0.0, "weight of the CRPS loss of the paired step (needs --supervised): G_A_B translates every paired "
                                  "input --crps_members times with codes from the step's prior draws, and the almost fair CRPS "
                                  "of those members against the paired B (ops.crps_loss) joins the generator loss, so that the "
                                  "ensemble's spread is trained and not only its median; 0: off; needs --norm instance and "
                                  "--grid_size up to 1024.  There is no lambda_crps_A: B -> A is deterministic, an ensemble of "
                                  "one, whose CRPS is the L1 term the step already has"),
    ("crps_members", int, 4, "members per paired input under --lambda_crps_B, 2..16 (at most the paired batch: member m of "
                             "input n is coded with the prior draw (n + m) mod batch); batch x members images go through G_A_B "
                             "in one pass and must fit it (255 images at 256 x 256 with --ngf 32)"),
    ("crps_alpha", float, 0.95, "under --lambda_crps_B: 1 is the fair CRPS (Ferro 2014), 0 the ensemble CRPS, between them the "
                                "almost fair score (Lang et al. 2024), which keeps a member from being sent away when the others "
                                "sit on the truth; inside [0, 1]"),
    ("native_res", "flag", False, "keep the fields at their stored resolution (no resize to --grid_size; both extents must be at "
                                  "least --grid_size): every training step cuts a fresh random --grid_size window per sample on "
                                  "the device (ops.window_gather), dev and test are cut once to their centre windows; whole "
                                  "fields are translated by model.translate_field / test.py --metric translate"),
    ("window_flip", ("choice", int, [0, 1]), 0, "with --native_res: 1 also mirrors every training window at random in x and y"),
]


class TrainOptions(object):
    def __init__(self):
        self.parser = argparse.ArgumentParser()
        self.initialized = False

    def initialize(self):
        self.parser.add_argument("--name", type=str, required=True, help="name of the experiment")
        for name, kind, default, text in _T:
            if kind == "flag":
                self.parser.add_argument("--" + name, action="store_true", help=text)
            elif isinstance(kind, tuple):
                self.parser.add_argument("--" + name, type=kind[1], choices=kind[2], default=default, help=text)
            else:
                self.parser.add_argument("--" + name, type=kind, default=default, help=text)
        self.initialized = True

    def parse(self, sub_dirs=None, argv=None):
        if not self.initialized:
            self.initialize()
        opt = self.opt = self.parser.parse_args(argv)
        if opt.dataroot is None and not opt.synthetic:
            self.parser.error("--dataroot is required (or --synthetic N)")
        if opt.defer_scalars and not opt.step_graph:
            self.parser.error("--defer_scalars requires --step_graph")
        g = opt.grid_size
        for fam in FAMILIES:                      # what every family refuses, from its record
            weights = [getattr(opt, o) for o in fam.options()]
            if not fam.negative_ok and any(w < 0 for w in weights):
                self.parser.error("%s must not be negative (got %s)" % (fam.flags(), ", ".join("%r" % w for w in weights)))
            if not fam.on(opt):
                continue
            if fam.paired_only and not opt.supervised:
                self.parser.error("%s: a term of the paired step, which requires --supervised" % fam.flags())
            if fam.paired_only and opt.model != "aug_cycle_gan":
                self.parser.error("%s: --model %s has no paired step (aug_cycle_gan has)" % (fam.flags(), opt.model))
            lo, hi, pow2, phrase = fam.grid
            if not lo <= g <= hi or (pow2 and g & (g - 1)):
                self.parser.error("%s: %s (--grid_size %d)" % (fam.flags(), phrase, g))
        if not 2 <= opt.crps_members <= 16:
            self.parser.error("--crps_members must lie in 2..16 (got %d)" % opt.crps_members)
        if not 0.0 <= opt.crps_alpha <= 1.0:
            self.parser.error("--crps_alpha must lie in [0, 1] (got %r)" % opt.crps_alpha)
        if BY_STEM["crps"].on(opt):
            if opt.norm != "instance":
                self.parser.error("--lambda_crps_B needs --norm instance: under batch statistics the members of one input "
                                  "would see each other (--norm %s)" % opt.norm)
            from .model import ensemble_chunk              # the step's own limit, met here before any data is loaded
            per_rank = max(opt.batchSize // max(int(os.environ.get("WORLD_SIZE", "1")), 1), 1)
            images, most = per_rank * min(opt.crps_members, per_rank), ensemble_chunk(opt.ngf, g, g)
            if images > most:
                self.parser.error("--lambda_crps_B: a paired batch of %d x %d members is %d images, more than the %d one pass of "
                                  "G_A_B holds at --grid_size %d with --ngf %d; lower --crps_members or --batchSize"
                                  % (per_rank, min(opt.crps_members, per_rank), images, most, g, opt.ngf))
        if not 0.0 < opt.fss_tau < float("inf"):
            self.parser.error("--fss_tau must be positive and finite (got %r)" % opt.fss_tau)
        if opt.native_res and opt.synthetic:
            self.parser.error("--native_res cuts windows from stored fields; --synthetic fields are --grid_size already")
        if opt.window_flip and not opt.native_res:
            self.parser.error("--window_flip 1 requires --native_res")
        if not 0.0 <= opt.ema_decay < 1.0:
            self.parser.error("--ema_decay must lie in [0, 1) (got %r)" % opt.ema_decay)
        opt.gpu_ids = [i for i in (int(tok) for tok in opt.gpu_ids.split(",")) if i >= 0]      # options.py:92-97
        if opt.gpu_ids and torch.cuda.is_available():
            local = int(os.environ.get("LOCAL_RANK", opt.gpu_ids[0]))
            torch.cuda.set_device(local)
            opt.gpu_ids = [local]
        opt.expr_dir = os.path.join(opt.checkpoints_dir, opt.name)
        os.makedirs(opt.expr_dir, exist_ok=True)
        args = vars(opt)
        banner = ["------------ Options -------------"]
        banner += ["%s: %s" % (str(k), str(args[k])) for k in sorted(args)]
        banner += ["-------------- End ----------------"]
        print("\n".join(banner))
        with open(os.path.join(opt.expr_dir, "opt.txt"), "wt") as f:                          # options.py:119-124
            f.write("\n".join(banner) + "\n")
        with open(os.path.join(opt.expr_dir, "opt.pkl"), "wb") as f:                          # options.py:126-128
            pickle.dump(args, f)
        if sub_dirs is not None:
            create_sub_dirs(opt, sub_dirs)
        return opt


REFERENCE_METRICS = ('bpp', 'mse', 'visual', 'noise_sens', 'mvgauss')      # the project's own: eval_metrics.METRICS


class TestOptions(object):
    """options.py:134-143 (the options of dtgan_amd.test).  Additions: the metric `mvgauss` (the reference's
    compute_bpp_MVGauss_B, test.py:143-153, reachable only by editing its source), --ubo_steps (test.py:246 hard-codes
    500) and --gpu_ids (test.py:214 hard-codes [0]); the metric `ensemble` with --n_samples and --quantiles; the metric
    `spectrum` and the metric `coherence` (both reuse --n_samples); the metric `fss` (reuses --n_samples) with
    --fss_quantiles, --fss_thresholds, --fss_windows and --fss_scales (the intensity-scale skill of the same events: the
    error split by dyadic scale); --ema 1 evaluates the checkpoint's averaged weights (every metric);
    the metric `translate` (whole fields at their stored resolution, reuses --n_samples) with --overlap; the metric
    `field_spectrum` (radial and cross spectra of those whole fields, reuses --n_samples and --overlap); the metric `ssim`
    (structural similarity of the paired translations, reuses --n_samples); the metric `marginal` (Wasserstein distances,
    quantiles and distribution functions of the fields' values, reuses --n_samples) with --marg_levels and --marg_bins; the
    metric `minkowski` (area, perimeter and Euler characteristic of the excursion sets, unpaired, reuses --n_samples) with
    --mink_bins, and --mink_components (the connected components of the same sets: objects, holes, object sizes); --fss_sal (with
    the metric `fss`: the SAL score, structure, amplitude and location of the objects of the same paired translations, into a
    file of its own) with --sal_quantiles, --sal_thresholds, --sal_floor and --sal_conn; --fss_rel (with the metric `fss`: the
    reliability tables of the ensemble's neighbourhood events - Brier score and its decomposition, reliability diagram, ROC -
    into a file of its own) with --rel_windows; --ens_maps (with the metric `ensemble`: per-cell climatology maps over the
    split - bias, RMSE, correlation in time, spread and skill, event frequencies and Brier score, value distributions - into
    a file of its own) with --map_quantiles, --map_thresholds, --map_bins and --map_levels."""

    def __init__(self):
        from .eval_metrics import METRICS      # here, not at the top: it imports train.py, which imports this module
        own = [m.name for m in METRICS]
        self.parser = argparse.ArgumentParser()
        self.parser.add_argument('--chk_path', required=True, type=str)
        self.parser.add_argument('--res_dir', type=str, default='test_res')
        self.parser.add_argument('--train_logvar', type=int, default=1)
        self.parser.add_argument('--dataroot', required=True, type=str)
        self.parser.add_argument('--metric', required=True, type=str, choices=list(REFERENCE_METRICS) + own)
        self.parser.add_argument('--ubo_steps', type=int, default=500, help='iterates of the variational bound per test batch')
        self.parser.add_argument('--gpu_ids', type=str, default='0', help='the GPU to evaluate on (the first id given)')
        self.parser.add_argument('--n_samples', type=_n_samples, default=16,
                                 help='--metric %s: translations per input (1..64)' % ' / '.join(own))
        self.parser.add_argument('--quantiles', type=_quantiles, default=(0.05, 0.5, 0.95),
                                 help='--metric ensemble: comma-separated quantile levels, sorted inside [0, 1], at most 8')
        self.parser.add_argument('--fss_quantiles', type=_fss_quantiles, default=(0.5, 0.9, 0.99),
                                 help='--metric fss: the event thresholds as quantile levels of the real training fields, per '
                                      'channel (trainB for A -> B, trainA for B -> A); comma-separated, inside [0, 1], at most 8')
        self.parser.add_argument('--fss_thresholds', type=_fss_thresholds, default=None,
                                 help='--metric fss: explicit event thresholds in data units, the same for every channel '
                                      '(comma-separated, at most 8); overrides --fss_quantiles')
        self.parser.add_argument('--fss_windows', type=_fss_windows, default=(1, 3, 5, 9, 17, 33),
                                 help='--metric fss: comma-separated odd neighbourhood widths in cells, at most 8; sorted, and 1 '
                                      '(the cell itself: bias, CSI, base rate) is put in front if absent')
        self.parser.add_argument('--fss_scales', type=int, choices=[0, 1], default=0,
                                 help='--metric fss: 1 also splits the error of the events by dyadic scale (intensity-scale skill '
                                      'score: MSE, skill and energy bias per threshold and scale 2^j); 0: off')
        self.parser.add_argument('--marg_levels', type=_marg_levels, default=(0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 0.999, 1.0),
                                 help='--metric marginal: comma-separated quantile levels inside [0, 1], at most 16')
        self.parser.add_argument('--marg_bins', type=_marg_bins, default=100,
                                 help='--metric marginal: B in 2..257; the distribution functions are compared at the B - 1 '
                                      'quantiles k / B of the real training fields, per channel (trainB for A -> B, trainA for '
                                      'B -> A)')
        self.parser.add_argument('--mink_bins', type=_mink_bins, default=32,
                                 help='--metric minkowski: B in 2..256; the excursion sets are taken at the B - 1 quantiles '
                                      'k / B of the real training fields, per channel (trainB for A -> B, trainA for B -> A)')
        self.parser.add_argument('--mink_components', type=int, choices=[0, 4, 8], default=0,
                                 help='--metric minkowski: 4 or 8 also labels the connected components of the excursion sets '
                                      'under that connectivity (counts, holes, sizes); 0: off')
        self.parser.add_argument('--fss_sal', type=int, choices=[0, 1], default=0,
                                 help='--metric fss: 1 also scores structure, amplitude and location of the objects of the '
                                      'paired translations (SAL) -> sal.npz; 0: off')
        self.parser.add_argument('--sal_quantiles', type=_sal_quantiles, default=(0.9,),
                                 help='--metric fss --fss_sal 1: the object thresholds as quantile levels of the real training fields, per '
                                      'channel (trainB for A -> B, trainA for B -> A); comma-separated, inside [0, 1], at most 8; '
                                      'sorted ascending before use')
        self.parser.add_argument('--sal_thresholds', type=_sal_thresholds, default=None,
                                 help='--metric fss --fss_sal 1: explicit object thresholds in data units, the same for every channel '
                                      '(comma-separated, finite, at most 8; sorted ascending); overrides --sal_quantiles')
        self.parser.add_argument('--sal_floor', type=_sal_floor, default=-1.0,
                                 help='--metric fss --fss_sal 1: the lower end of the data range; the mass of a cell is its amount above it '
                                      '(finite, default -1)')
        self.parser.add_argument('--sal_conn', type=int, choices=[4, 8], default=8,
                                 help='--metric fss --fss_sal 1: the connectivity of the objects, 4 (shared edges) or 8 (edges or corners)')
        self.parser.add_argument('--fss_rel', type=int, choices=[0, 1], default=0,
                                 help='--metric fss: 1 also counts, per number of members in the neighbourhood event, the cells '
                                      'where the truth has it (Brier score, reliability, resolution, ROC) -> reliability.npz; 0: off')
        self.parser.add_argument('--rel_windows', type=_rel_windows, default=(1, 5, 17),
                                 help='--metric fss --fss_rel 1: comma-separated odd neighbourhood widths in cells, at most 8, each '
                                      'at most 65; the neighbourhood event of a cell is any event inside the window')
        self.parser.add_argument('--ens_maps', type=int, choices=[0, 1], default=0,
                                 help='--metric ensemble: 1 also accumulates, per cell of the grid across the split, the moments, '
                                      'event counts and histograms of the members against the truth (bias, RMSE, correlation, '
                                      'spread/skill, Brier, quantile maps) -> ensemble_maps.npz; 0: off')
        self.parser.add_argument('--map_quantiles', type=_map_quantiles, default=(0.9, 0.99),
                                 help='--metric ensemble --ens_maps 1: the event thresholds as quantile levels of the real training '
                                      'fields, per channel (trainB for A -> B, trainA for B -> A); comma-separated, inside [0, 1], at '
                                      'most 8, sorted ascending before use; "none": no events')
        self.parser.add_argument('--map_thresholds', type=_map_thresholds, default=None,
                                 help='--metric ensemble --ens_maps 1: explicit event thresholds in data units, the same for every '
                                      'channel (comma-separated, finite, at most 8; sorted ascending); overrides --map_quantiles')
        self.parser.add_argument('--map_bins', type=_map_bins, default=32,
                                 help='--metric ensemble --ens_maps 1: B = 0 (no histograms) or in 2..64; every cell keeps a histogram '
                                      'of its values between the B - 1 quantiles k / B of the real training fields, per channel')
        self.parser.add_argument('--map_levels', type=_map_levels, default=(0.5, 0.95, 0.99),
                                 help='--metric ensemble --ens_maps 1: comma-separated quantile levels inside [0, 1], at most 16, of '
                                      'the per-cell quantile maps (resolved to the histogram edges)')
        self.parser.add_argument('--overlap', type=_overlap, default=None,
                                 help='--metric translate / field_spectrum: pixels neighbouring windows share, 0 .. grid_size // 2 '
                                      '(default: grid_size // 4)')
        self.parser.add_argument('--ema', type=int, choices=[0, 1], default=0,
                                 help='1: every metric runs on the averaged weights the checkpoint holds under ema_<net> '
                                      '(a run trained with --ema_decay); 0: on the live weights')

    def parse(self, argv=None):
        return self.parser.parse_args(argv)


def _n_samples(s):
    v = int(s)
    if not 1 <= v <= 64:
        raise argparse.ArgumentTypeError("--n_samples must lie in 1..64 (got %d)" % v)
    return v


def _overlap(s):
    v = int(s)
    if v < 0:
        raise argparse.ArgumentTypeError("--overlap must lie in 0 .. grid_size // 2 (got %d)" % v)
    return v


def check_overlap(overlap, grid_size):
    """--overlap against the run's grid_size (known only once the saved options are read) -> the overlap in pixels
    (None: grid_size // 4); ValueError outside 0 .. grid_size // 2"""
    if overlap is None:
        return grid_size // 4
    if not 0 <= overlap <= grid_size // 2:
        raise ValueError("--overlap must lie in 0 .. grid_size // 2 = %d (got %d)" % (grid_size // 2, overlap))
    return int(overlap)


def _split(name, s, kind, noun):
    try:
        return [kind(t) for t in s.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError("%s: not a comma-separated list of %s: %r" % (name, noun, s))


def _floats(name, ok, rule, ordered=False, most=8):
    """the argparse type of a comma-separated list of 1 to `most` floats that each pass `ok`, ascending where `ordered`;
    `rule` words the refusal"""
    def parse(s):
        v = tuple(_split(name, s, float, "numbers"))
        if not 1 <= len(v) <= most or not all(ok(x) for x in v) or (ordered and any(b < a for a, b in zip(v, v[1:]))):
            raise argparse.ArgumentTypeError("%s: 1 to %d %s (got %r)" % (name, most, rule, s))
        return v
    return parse


_level = lambda x: 0.0 <= x <= 1.0
_quantiles = _floats("--quantiles", _level, "levels, sorted inside [0, 1]", ordered=True)
_fss_quantiles = _floats("--fss_quantiles", _level, "levels inside [0, 1]")
_fss_thresholds = _floats("--fss_thresholds", lambda x: x == x, "numbers")
_marg_levels = _floats("--marg_levels", _level, "levels inside [0, 1]", most=16)
_finite = lambda x: x - x == 0.0


def _sorted(parse):
    return lambda s: tuple(sorted(parse(s)))


_sal_quantiles = _sorted(_floats("--sal_quantiles", _level, "levels inside [0, 1]"))
_sal_thresholds = _sorted(_floats("--sal_thresholds", _finite, "finite numbers"))


_map_thresholds = _sorted(_floats("--map_thresholds", _finite, "finite numbers"))
_map_levels = _floats("--map_levels", _level, "levels inside [0, 1]", most=16)


def _map_quantiles(s):
    return () if s.strip().lower() == "none" else _sorted(_floats("--map_quantiles", _level, "levels inside [0, 1]"))(s)


def _map_bins(s):
    v = int(s)
    if v != 0 and not 2 <= v <= 64:
        raise argparse.ArgumentTypeError("--map_bins must be 0 or lie in 2..64 (got %d)" % v)
    return v


def _sal_floor(s):
    v = float(s)
    if not _finite(v):
        raise argparse.ArgumentTypeError("--sal_floor must be finite (got %r)" % s)
    return v


def _marg_bins(s):
    v = int(s)
    if not 2 <= v <= 257:
        raise argparse.ArgumentTypeError("--marg_bins must lie in 2..257 (got %d)" % v)
    return v


def _mink_bins(s):
    v = int(s)
    if not 2 <= v <= 256:
        raise argparse.ArgumentTypeError("--mink_bins must lie in 2..256 (got %d)" % v)
    return v


def _fss_windows(s):
    w = sorted(set(_split("--fss_windows", s, int, "integers")))
    if not w or any(v < 1 or v % 2 == 0 for v in w):
        raise argparse.ArgumentTypeError("--fss_windows: odd positive widths (got %r)" % s)
    if w[0] != 1:
        w.insert(0, 1)
    if len(w) > 8:
        raise argparse.ArgumentTypeError("--fss_windows: at most 8 widths, 1 included (got %r)" % s)
    return tuple(w)


def _rel_windows(s):
    w = tuple(_split("--rel_windows", s, int, "integers"))
    if not 1 <= len(w) <= 8 or any(v < 1 or v % 2 == 0 or v > 65 for v in w):
        raise argparse.ArgumentTypeError("--rel_windows: 1 to 8 odd widths of at most 65 cells (got %r)" % s)
    return w


def _fss_loss_windows(s):
    w = tuple(_split("--fss_loss_windows", s, int, "integers"))
    if not 1 <= len(w) <= 8 or any(v < 1 or v % 2 == 0 or v > 65 for v in w):
        raise argparse.ArgumentTypeError("--fss_loss_windows: 1 to 8 odd widths of at most 65 cells (got %r)" % s)
    return w


# the fractions-skill-score loss of the paired step; here because its list types are the helpers above
_T += [
    ("lambda_fss_A", float, 0.0, "weight of the fractions-skill-score loss of the paired step (needs --supervised) on the paired "
                                 "prediction of A against the real A: 1 - FSS of soft threshold exceedances (ops.fss_loss: "
                                 "sigmoid((x - threshold) / --fss_tau), summed over --fss_loss_windows, pooled over the batch), "
                                 "which rewards putting a rare event nearly in the right place; 0: off (with --lambda_fss_B on, "
                                 "this side is reported as S_fss_A without a gradient); needs --grid_size up to 1024"),
    ("lambda_fss_B", float, 0.0, "the same on the paired prediction of B against the real B"),
    ("fss_loss_quantiles", _floats("--fss_loss_quantiles", _level, "levels inside [0, 1]"), (0.9, 0.99),
     "under --lambda_fss_A / --lambda_fss_B: the event thresholds as quantile levels of the real training fields, per channel "
     "(the climatology --metric fss uses); comma-separated, inside [0, 1], at most 8"),
    ("fss_loss_thresholds", _floats("--fss_loss_thresholds", lambda x: x == x and abs(x) != float("inf"), "finite numbers"), None,
     "explicit event thresholds of the loss in data units, the same for every channel (comma-separated, at most 8); overrides "
     "--fss_loss_quantiles"),
    ("fss_loss_windows", _fss_loss_windows, (3, 9, 17), "comma-separated odd neighbourhood widths of the loss in cells, each at "
                                                       "most 65, at most 8 of them"),
    ("fss_tau", float, 0.05, "the temperature of the soft events in data units (fields in [-1, 1]): smaller is closer to the "
                             "evaluator's hard events and gives a gradient to fewer cells; must be positive"),
]
