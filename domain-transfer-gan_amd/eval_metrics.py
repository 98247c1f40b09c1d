"""The evaluator's own metrics (python -m dtgan_amd.test --metric ensemble ... minkowski): what each one is stands in ONE record
of METRICS - its name, how its data is loaded and batched, what it derives from the training data before the splits
(prepare), the line it prints (report) and its paragraph of test.py's documentation - next to the eval_* function that
scores one split.  test.test_model looks the record up and runs prepare, _eval_splits and report; options.TestOptions takes
the names from the table.  Adding a metric: its record, its eval_*, its model.translate_* and its options.

What the eval_* functions share: _batches (a split's batches on the device), _domain_tables (per-domain tables uploaded at
the first batch), _Sum (sums over a split in float64 / int64) and _read_back (one device->host copy per batch)."""
import os
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .dataloader import AlignedIterator
from .evaluate import one_to_three_channels
from .train import save_image_grid


def _read_back(tensors):
    """device tensors of one dtype -> host arrays of their shapes, through ONE device->host copy"""
    tensors = list(tensors)
    host = torch.cat([t.reshape(-1) for t in tensors]).cpu().numpy()
    ends = np.cumsum([t.numel() for t in tensors])
    return [host[e - t.numel():e].reshape(tuple(t.shape)) for e, t in zip(ends, tensors)]


def _batches(dataset, use_gpu=True):
    """(real_A, real_B) of every batch of a split, on the device where use_gpu"""
    for batch in dataset:
        real_A, real_B = batch['A'], batch['B']
        if use_gpu:
            real_A, real_B = real_A.cuda(), real_B.cuda()
        yield real_A, real_B


def _domain_tables(table_B, table_A, check=None):
    """two per-domain host tables (C, T) -> on_device(real_B, real_A) -> (table_B, table_A) as tensors on the devices of B and
    A, uploaded once, at the first batch.  check(table, C): what makes a table a contiguous array first (default: as it is)"""
    dev = []

    def on_device(real_B, real_A):
        if not dev:
            for table, side in ((table_B, real_B), (table_A, real_A)):
                table = np.ascontiguousarray(table) if check is None else check(table, side.size(1))
                dev.append(torch.from_numpy(table).to(side.device))
        return dev
    return on_device


class _Sum(object):
    """The sum of arrays over their leading axis, batch by batch in the order they come: integers in int64, everything else
    in float64.  total: the sum; rows: how many entries of the leading axis went in; cells: rows times what each holds"""

    def __init__(self):
        self.total, self.rows, self.cells = 0, 0, 0

    def add(self, v, cells_per_row=0, keep=None, rows=None):
        """v (rows, ...), or with keep any leading axes in front of the last `keep`.  rows: what to count where v is the
        sum of that many rows already (v then has a leading axis of 1)"""
        if keep is not None:
            v = v.reshape((-1,) + v.shape[v.ndim - keep:])
        self.total = self.total + (v.sum(0, dtype=np.int64) if v.dtype.kind in 'iu' else v.astype(np.float64).sum(0))
        rows = v.shape[0] if rows is None else rows
        self.rows += rows
        self.cells += rows * cells_per_row


def _cells(t):
    return t.size(2) * t.size(3)


ENSEMBLE_SCORES = ('crps', 'crps_fair', 'mse_mean', 'spread', 'coverage')


MAP_PAIRS = ('members_B', 'fake_A')
MAP_STATE_LIMIT = 2 << 30          # bytes of whole-split per-cell state on the device
_MAP_PARTS = ('mom', 'evt', 'hist_x', 'hist_y')


def plan_ens_maps(opt, arrays):
    """--ens_maps 1: what the per-cell maps need before a split is touched -> the record eval_ensemble_B takes as `maps`:
    thresholds_B / thresholds_A (C, T) float32 or None (fss_thresholds of --map_quantiles / --map_thresholds on trainB /
    trainA), edges_B / edges_A (C, B - 1) float32 or None (marginal_edges of --map_bins), levels.  arrays = (trainA, trainB,
    devA, devB, testA, testB).  ValueError for a state of both directions above MAP_STATE_LIMIT on the device, and for a
    split whose rows times --n_samples pass the 2^31 - 1 an int32 histogram count holds."""
    trainA, trainB, devA, devB, testA, testB = arrays
    quant, explicit, bins = tuple(opt.map_quantiles), opt.map_thresholds, int(opt.map_bins)
    tables = {}
    for d, train in (('B', trainB), ('A', trainA)):
        none = explicit is None and not quant
        tables['thresholds_' + d] = None if none else fss_thresholds(train, quant, explicit)
        tables['edges_' + d] = marginal_edges(train, bins) if bins else None
    T = 0 if tables['thresholds_B'] is None else tables['thresholds_B'].shape[1]
    if T > ops.CELL_MAX_T or not (bins == 0 or 2 <= bins <= ops.CELL_MAX_E + 1):
        raise ValueError("--ens_maps: at most %d thresholds and --map_bins 0 or in 2..%d (got %d, %d)"
                         % (ops.CELL_MAX_T, ops.CELL_MAX_E + 1, T, bins))
    E = max(bins - 1, 0)
    need = sum(ops.cell_state_bytes(np.shape(a)[1], np.shape(a)[2], np.shape(a)[3], T, E) for a in (devB, devA))
    if need > MAP_STATE_LIMIT:
        raise ValueError("--ens_maps: the per-cell state of a split needs %d bytes (%.2f GiB) on the device, above %d GiB; fewer "
                         "--map_bins (0: no histograms) and fewer --map_quantiles / --map_thresholds shrink it"
                         % (need, need / float(1 << 30), MAP_STATE_LIMIT >> 30))
    rows = max(len(devB), len(testB)) * int(opt.n_samples)
    if rows > 2 ** 31 - 1:
        raise ValueError("--ens_maps: %d member rows per cell pass the 2^31 - 1 an int32 histogram count holds" % rows)
    tables['levels'] = tuple(opt.map_levels)
    return tables


def _maps_result(states, crps_sum, maps):
    """the states of MAP_PAIRS (device) -> the entries of a split in ensemble_maps.npz: per pair k the raw state (mom_k, evt_k,
    hist_x_k, hist_y_k, n_k, members_k) and every map of ops.cell_summary as <map>_k; crps_B.  One copy per dtype"""
    host = {k: dict(n=states[k]['n'], M=states[k]['M']) for k in MAP_PAIRS}
    for part in _MAP_PARTS:
        have = [k for k in MAP_PAIRS if states[k][part] is not None]
        extra = [crps_sum] if part == 'mom' else []
        got = _read_back([states[k][part] for k in have] + extra) if have else []
        for k, v in zip(have, got):
            host[k][part] = v
        for k in MAP_PAIRS:
            host[k].setdefault(part, None)
        if extra:
            crps = got[-1]
    res = {'crps_B': crps / float(max(host['members_B']['n'], 1))}
    for k in MAP_PAIRS:
        d = k[-1]
        res.update(('%s_%s' % (part, k), host[k][part]) for part in _MAP_PARTS if host[k][part] is not None)
        res['n_' + k], res['members_' + k] = np.int64(host[k]['n']), np.int64(host[k]['M'])
        summary = ops.cell_summary(host[k], maps['thresholds_' + d], maps['edges_' + d], maps['levels'])
        res.update(('%s_%s' % (name, k), v) for name, v in summary.items())
    return res


def eval_ensemble_B(dataset, model, n_samples, quantiles, use_gpu=True, maps=None):
    """the per-input ensemble scores of A -> B on an aligned split (model.translate_ensemble, one read of the numbers per
    batch) -> ({score: (N,) array for every input}, rank histogram pooled over the split (n_samples + 1,)).
    maps: None, or the record of plan_ens_maps: the per-cell statistics of the same members too (ops.cell_stats after every
    group's ensemble_stats, no random draw more; the state lives on the device for the whole split), and of B -> A
    (model.translate_cell_stats_A), and the return gains a third entry, the dict of _maps_result"""
    per, hist = {k: [] for k in ENSEMBLE_SCORES}, np.zeros(n_samples + 1, dtype=np.int64)
    states, crps_sum, tables = None, None, None
    for real_A, real_B in _batches(dataset, use_gpu):
        cell = None
        if maps is not None:
            if states is None:
                T = 0 if maps['thresholds_B'] is None else maps['thresholds_B'].shape[1]
                E = 0 if maps['edges_B'] is None else maps['edges_B'].shape[1]
                states = {k: ops.cell_state(t.size(1), t.size(2), t.size(3), T, E, t.device)
                          for k, t in zip(MAP_PAIRS, (real_B, real_A))}
                up = lambda a, t: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(t.device)
                tables = {d: (up(maps['thresholds_' + d], t), up(maps['edges_' + d], t)) for d, t in (('B', real_B), ('A', real_A))}
                crps_sum = torch.zeros(real_B.shape[1:], dtype=torch.float64, device=real_B.device)
            cell = (states['members_B'],) + tables['B']
        r = model.translate_ensemble(real_A, n_samples, real_B=real_B, quantiles=quantiles, cell_stats=cell)
        *scores, ranks = _read_back([r[k].double() for k in ENSEMBLE_SCORES + ('rank_hist',)])
        for k, v in zip(ENSEMBLE_SCORES, scores):
            per[k].append(v)
        hist += ranks.sum(0).astype(np.int64)
        if maps is not None:
            crps_sum += r['crps_map'].double().sum(0)
            model.translate_cell_stats_A(real_B, real_A, states['fake_A'], *tables['A'])
    res = {k: np.concatenate(v) for k, v in per.items()}, hist
    return res if maps is None else res + (_maps_result(states, crps_sum, maps),)


def visualize_ensemble(opt, real_A, real_B, model, name):
    """rows A, B, ensemble mean, std (scaled to the image range by the grid's largest value), lowest and highest quantile;
    one column per input"""
    r = model.translate_ensemble(real_A, opt.n_samples, quantiles=opt.quantiles)
    std = r['std']
    std = std * (2. / max(float(std.max()), 1e-12)) - 1.
    rows = [real_A, real_B, r['mean'], std, r['quantiles'][:, 0], r['quantiles'][:, -1]]
    grid = torch.cat([one_to_three_channels(x.detach().cpu()) for x in rows], 0)
    save_image_grid(grid.float()[:, :3], os.path.join(opt.res_dir, name), real_A.size(0))


def log_spectral_distance(p, q):
    """(..., C, nb) spectra -> (...,) float64: sqrt(mean over bins 1 .. S/2 of (10 log10(p / q))^2) in dB, both clamped at
    1e-30, averaged over the channels"""
    p = np.maximum(np.asarray(p, dtype=np.float64)[..., 1:], 1e-30)
    q = np.maximum(np.asarray(q, dtype=np.float64)[..., 1:], 1e-30)
    return np.sqrt(np.mean((10.0 * np.log10(p / q)) ** 2, axis=-1)).mean(axis=-1)


def _lsd_entries(res):
    """the distances of the split-mean spectra res holds under psd_*: lsd_B, lsd_mean_B, lsd_A"""
    return dict(lsd_B=float(log_spectral_distance(res['psd_members_B'], res['psd_real_B'])),
                lsd_mean_B=float(log_spectral_distance(res['psd_ens_mean_B'], res['psd_real_B'])),
                lsd_A=float(log_spectral_distance(res['psd_fake_A'], res['psd_real_A'])))


def eval_spectrum(dataset, model, n_samples, use_gpu=True):
    """radially averaged power spectra on an aligned split, one read of the bin arrays per batch.  A -> B: n_samples members
    per input and their ensemble mean (model.translate_spectrum) against the real B; B -> A: predict_A against the real A.
    -> dict: psd_real_B, psd_members_B (over inputs and members), psd_ens_mean_B, psd_real_A, psd_fake_A: split means, (C, nb)
    float64; lsd_B, lsd_mean_B, lsd_A: the distances of those means; lsd_B_per_input (N,): every input's member-mean
    spectrum against its own paired B"""
    keys = ('members', 'ens_mean', 'target', 'real_A', 'fake_A')
    parts = {k: [] for k in keys}
    for real_A, real_B in _batches(dataset, use_gpu):
        r = model.translate_spectrum(real_A, n_samples, real_B=real_B)
        with torch.no_grad():
            r['fake_A'] = ops.radial_spectrum(model.predict_A(real_B), real_A.size(1), "nchw")
        r['real_A'] = ops.radial_spectrum(real_A, real_A.size(1), "nchw")
        for k, v in zip(keys, _read_back([r[k] for k in keys])):
            parts[k].append(v.astype(np.float64))
    p = {k: np.concatenate(v) for k, v in parts.items()}
    res = dict(psd_real_B=p['target'].mean(0), psd_members_B=p['members'].mean((0, 1)), psd_ens_mean_B=p['ens_mean'].mean(0),
               psd_real_A=p['real_A'].mean(0), psd_fake_A=p['fake_A'].mean(0))
    res.update(_lsd_entries(res))
    res['lsd_B_per_input'] = log_spectral_distance(p['members'].mean(1), p['target'])
    return res


COHERENCE_PAIRS = ('members_B', 'ens_mean_B', 'fake_A')


def _cross_spectra(dataset, translate_B, triples_A, use_gpu):
    """The split loop of eval_coherence and eval_field_spectrum -> {k: _Sum of the (pxx, pyy, cxy) triples (C, 3, nb)} per
    comparison k of COHERENCE_PAIRS, summed over the split (over the members too) before anything is divided, one read of the
    bin arrays per batch.  translate_B(real_A, real_B) -> the model's dict of members and ens_mean against the paired B;
    triples_A(real_A, real_B) -> the triples of B -> A against the paired A"""
    sums = {k: _Sum() for k in COHERENCE_PAIRS}
    for real_A, real_B in _batches(dataset, use_gpu):
        r = translate_B(real_A, real_B)
        parts = (r['members'].flatten(0, 1), r['ens_mean'], triples_A(real_A, real_B))
        for k, v in zip(COHERENCE_PAIRS, _read_back(parts)):
            sums[k].add(v)
    return sums


def _coherence_entries(sums):
    """per comparison k of COHERENCE_PAIRS: the summed triples sums_k and ops.coherence_summary of them, perr_k per pair"""
    res = {}
    for k in COHERENCE_PAIRS:
        res['sums_' + k] = sums[k].total
        summary = ops.coherence_summary(sums[k].total)
        summary['perr'] = summary['perr'] / sums[k].rows
        res.update(('%s_%s' % (name, k), v) for name, v in summary.items())
    return res


def eval_coherence(dataset, model, n_samples, use_gpu=True):
    """paired cross-spectra on an aligned split, one read of the bin arrays per batch.  A -> B: n_samples members per input
    and their ensemble mean (model.translate_coherence) against the paired real B; B -> A: predict_A against the paired real
    A.  The (pxx, pyy, cxy) triples of every comparison are summed over the split (over the members too) before anything is
    divided: one pair's ring-wise coherence is noisy where a ring has few cells.  -> dict, per comparison k of
    COHERENCE_PAIRS: sums_k (C, 3, nb) float64 and coh_k, r_k, perr_k (C, nb), k_eff_k (C,) of ops.coherence_summary; perr_k
    is the mean error spectrum per pair (the summed one over the number of pairs)"""
    def fake_A(real_A, real_B):
        with torch.no_grad():
            return ops.cross_spectrum(model.predict_A(real_B), real_A, real_A.size(1), "nchw", "nchw")
    return _coherence_entries(_cross_spectra(dataset, lambda a, b: model.translate_coherence(a, n_samples, b), fake_A, use_gpu))


def eval_field_spectrum(dataset, model, n_samples, overlap, use_gpu=True):
    """whole-field cross-spectra of an aligned split at its stored resolution, one read of the bin arrays per batch.  A -> B:
    n_samples tiled translations per field and their per-pixel mean (model.translate_field_spectrum) against the paired whole
    real B; B -> A: translate_field_A against the paired whole real A.  The (pxx, pyy, cxy) triples of every comparison are
    summed over the split (over the members too) in float64 before anything is divided.  -> dict: per comparison k of
    COHERENCE_PAIRS what eval_coherence gives (sums_k, coh_k, r_k, perr_k, k_eff_k); the split-mean spectra the triples carry,
    (C, nb) float64: psd_members_B, psd_ens_mean_B, psd_fake_A (pxx) and psd_real_B, psd_real_A (pyy, once per input); and the
    distances lsd_B, lsd_mean_B, lsd_A of those means"""
    def fake_A(real_A, real_B):
        return ops.field_cross_spectrum(model.translate_field_A(real_B, overlap=overlap), real_A, real_A.size(1), "nchw", "nchw")
    sums = _cross_spectra(dataset, lambda a, b: model.translate_field_spectrum(a, n_samples, b, overlap=overlap), fake_A, use_gpu)
    res = _coherence_entries(sums)
    for k in COHERENCE_PAIRS:
        res['psd_' + k] = sums[k].total[:, 0] / sums[k].rows
    res['psd_real_B'] = sums['ens_mean_B'].total[:, 1] / sums['ens_mean_B'].rows
    res['psd_real_A'] = sums['fake_A'].total[:, 1] / sums['fake_A'].rows
    res.update(_lsd_entries(res))
    return res


SSIM_PAIRS = ('members_B', 'ens_mean_B', 'fake_A')


def eval_ssim(dataset, model, n_samples, use_gpu=True):
    """structural similarity on an aligned split, one read of the (S, cs) pairs per batch.  A -> B: n_samples members per
    input and their ensemble mean (model.translate_ssim) against the paired real B; B -> A: predict_A against the paired real
    A.  -> dict, per comparison k of SSIM_PAIRS, float64: ssim_k, cs_k (C,), the means over the split (and the members), and
    ssim_k_per_input, cs_k_per_input (N, C), the members averaged per input"""
    parts = {k: [] for k in SSIM_PAIRS}
    for real_A, real_B in _batches(dataset, use_gpu):
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
    """eval_marginal's result from what its batches gave.  parts[k], per comparison k of MARGINAL_PAIRS: w, a list of
    (n, C, 2) float64 (the members averaged per input), and the _Sums q (C, L) float64 over the fields and below (C, E) int64
    with the cells they run over; real['B'], real['A']: q and below of the paired real fields of that direction"""
    res = {}

    def pooled(name, p):
        res['q_' + name] = p['q'].total / float(p['q'].rows)
        res['below_' + name], res['cells_' + name] = np.asarray(p['below'].total, dtype=np.int64), np.int64(p['below'].cells)
    for k in MARGINAL_PAIRS:
        p, r = parts[k], real[k[-1]]
        w = np.concatenate(p['w'])                                 # (N, C, 2)
        res['w1_' + k], res['w2sq_' + k] = w[..., 0].mean(0), w[..., 1].mean(0)
        res['w1_%s_per_input' % k], res['w2sq_%s_per_input' % k] = w[..., 0], w[..., 1]
        pooled(k, p)
        summary = ops.marginal_summary(p['below'].total, p['below'].cells, r['below'].total, r['below'].cells)
        res['cdf_' + k], res['ks_' + k] = summary['cdf'], summary['ks']
    for d in ('B', 'A'):
        pooled('real_' + d, real[d])
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
    zero = lambda: dict(w=[], q=_Sum(), below=_Sum())
    parts, real = {k: zero() for k in MARGINAL_PAIRS}, {d: zero() for d in ('B', 'A')}
    edges = _domain_tables(edges_B, edges_A)
    for real_A, real_B in _batches(dataset, use_gpu):
        e_B, e_A = edges(real_B, real_A)
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
        accs = [parts[k] for k in MARGINAL_PAIRS] + [real['B'], real['A']]
        cells = [_cells(real_B), _cells(real_B), _cells(real_A), _cells(real_B), _cells(real_A)]
        for i, acc in enumerate(accs):       # q (..., C, L) and below (..., C, E) of some fields, over their leading axes
            acc['q'].add(rest[2 * i], keep=2)
            acc['below'].add(rest[2 * i + 1].astype(np.int64), cells[i], keep=2)
        for i, k in enumerate(MARGINAL_PAIRS):
            parts[k]['w'].append(w[i].mean(1) if k == 'members_B' else w[i])
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


REL_PAIRS = ('ens_prob_B', 'members_B', 'ens_mean_B', 'fake_A')


def eval_fss(dataset, model, n_samples, thresholds_B, thresholds_A, windows, use_gpu=True, scales=False, reliability=None):
    """fractions-skill-score triples on an aligned split, one read of the sums per batch.  A -> B: n_samples members per
    input, the ensemble as a probability and the ensemble mean (model.translate_fss) against the paired real B; B -> A:
    predict_A against the paired real A.  The int64 triples of every comparison are summed over the split (over the members
    too) before anything is divided.  -> dict, per comparison k of FSS_PAIRS: sums_k (C, T, nw, 3) int64 and fss_k (C, T, nw),
    bias_k, csi_k, base_rate_k (C, T), useful_scale_k (C, T) int64 of ops.fss_summary (ens_prob_B with members=n_samples).
    scales: the intensity-scale triples of the same events too (ops.fss_scales; nl dyadic levels), summed like the others: per
    k scale_sums_k (C, T, nl, 3) int64 and mse_scale_k, iss_k, en_rel_k (C, T, nl), mse_random_k (C, T), skill_scale_k (C, T)
    int64 of ops.fss_scale_summary (ens_prob_B with members=n_samples and the members' events); False: none of them, and no
    launch more than before.
    reliability: None, or a tuple of odd windows of at most 65: the reliability tables of the same events too (ops.reliability;
    the same members, no random draw more), and the return is the pair (the dict above, rel): per comparison k of REL_PAIRS
    table_k, the int64 tables summed over the split (ens_prob_B (C, T, nwr, M + 1, 2): cells by the number of members in the
    neighbourhood event and by the truth's; the others (C, T, nwr, 2, 2), members_B summed over the members too), and every
    entry of ops.reliability_summary as <entry>_k"""
    sums = {k: _Sum() for k in FSS_PAIRS}
    tables = {k: _Sum() for k in REL_PAIRS}
    scale = {k: _Sum() for k in FSS_PAIRS}
    thresholds = _domain_tables(thresholds_B, thresholds_A)
    for real_A, real_B in _batches(dataset, use_gpu):
        thr_B, thr_A = thresholds(real_B, real_A)
        r = model.translate_fss(real_A, n_samples, real_B, thr_B, windows, scales=scales, reliability=reliability)
        with torch.no_grad():
            pred_A = model.predict_A(real_B)
            fake_A = ops.fss(pred_A, real_A, real_A.size(1), "nchw", "nchw", thr_A, windows)
        parts = (r['members'].flatten(0, 1), r['ens_prob'], r['ens_mean'], fake_A)
        for k, v in zip(FSS_PAIRS, _read_back(parts)):
            sums[k].add(v, _cells(real_B))
        if scales:
            parts = (r['members_scale'].flatten(0, 1), r['ens_prob_scale'], r['ens_mean_scale'],
                     ops.fss_scales(pred_A, real_A, real_A.size(1), "nchw", "nchw", thr_A))
            for k, v in zip(FSS_PAIRS, _read_back(parts)):
                scale[k].add(v)
        if reliability is not None:
            parts = (r['ens_rel'], r['members_rel'].flatten(0, 1), r['ens_mean_rel'],
                     ops.reliability(pred_A, real_A, real_A.size(1), "nchw", "nchw", thr_A, reliability))
            for k, v in zip(REL_PAIRS, _read_back(parts)):
                tables[k].add(v)
    res = {}
    for k in FSS_PAIRS:
        res['sums_' + k] = np.asarray(sums[k].total, dtype=np.int64)
        summary = ops.fss_summary(sums[k].total, windows, sums[k].cells, members=n_samples if k == 'ens_prob_B' else 1)
        res.update(('%s_%s' % (name, k), v) for name, v in summary.items())
    if scales:
        for k in FSS_PAIRS:
            res['scale_sums_' + k] = np.asarray(scale[k].total, dtype=np.int64)
            ens = dict(members=n_samples, forecast_events=scale['members_B'].total[..., 0, 0]) if k == 'ens_prob_B' else {}
            summary = ops.fss_scale_summary(scale[k].total, sums[k].cells, **ens)
            res.update(('%s_%s' % ('mse_scale' if name == 'mse' else name, k), v) for name, v in summary.items())
    if reliability is None:
        return res
    rel = {}
    for k in REL_PAIRS:
        rel['table_' + k] = np.asarray(tables[k].total, dtype=np.int64)
        rel.update(('%s_%s' % (name, k), v) for name, v in ops.reliability_summary(rel['table_' + k]).items())
    return res, rel


SAL_PAIRS = ('members_B', 'ens_mean_B', 'fake_A')
SAL_SCORES = ('S', 'A', 'L1', 'L2', 'L')


def _nan_reduce(fn, v):
    """fn (np.nanmedian, np.nanmean) over the leading axis of v; NaN, silently, where nothing is defined"""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return fn(v, axis=0)


def eval_sal(dataset, model, n_samples, thresholds_B, thresholds_A, floor=-1.0, conn=8, use_gpu=True):
    """the SAL scores (Wernli et al. 2008) on an aligned split, one read of the integers and one of the doubles per batch.
    A -> B: n_samples members per input and their ensemble mean against the paired real B (model.translate_sal); B -> A:
    predict_A against the paired real A (ops.sal on both).  Every pair is scored on its own (ops.sal_scores, float64 on the
    host).  -> dict, per comparison k of SAL_PAIRS: the per-input arrays S_k, L2_k, L_k (N, [M,] C, T) and A_k, L1_k
    (N, [M,] C) (M: members_B only); over the pairs of the split (and the members), NaN-aware: median_S_k, median_L_k,
    mean_abs_S_k, mean_L_k (C, T) and median_A_k, mean_abs_A_k (C,); defined_k (C, T): the fraction of pairs whose S and L
    are not NaN"""
    parts = {k: {s: [] for s in SAL_SCORES} for k in SAL_PAIRS}
    thresholds = _domain_tables(thresholds_B, thresholds_A, check=ops.check_thresholds)
    kw = dict(floor=floor, conn=conn)
    names = ('field', 'obj', 'shape')
    for real_A, real_B in _batches(dataset, use_gpu):
        thr_B, thr_A = thresholds(real_B, real_A)
        r = model.translate_sal(real_A, n_samples, real_B, thr_B, **kw)
        CA = real_A.size(1)
        with torch.no_grad():
            fake_A = ops.sal(model.predict_A(real_B), CA, "nchw", thr_A, **kw)
        true_A = ops.sal(real_A, CA, "nchw", thr_A, **kw)
        sets = [tuple(r['%s_%s' % (who, n)] for n in names) for who in ('members', 'ens_mean', 'target')] + [fake_A, true_A]
        ints = _read_back([t for s in sets for t in s[:2]])
        dbls = _read_back([s[2] for s in sets])
        mem, mean, tgt, fa, ta = [(ints[2 * i], ints[2 * i + 1], dbls[i]) for i in range(len(sets))]
        H, W = real_B.shape[-2:]
        pairs = (ops.sal_scores(mem, tuple(a[:, None] for a in tgt), H, W), ops.sal_scores(mean, tgt, H, W),
                 ops.sal_scores(fa, ta, *real_A.shape[-2:]))
        for k, sc in zip(SAL_PAIRS, pairs):
            for s in SAL_SCORES:
                parts[k][s].append(sc[s])
    res = {}
    for k in SAL_PAIRS:
        p = {s: np.concatenate(v) for s, v in parts[k].items()}
        res.update(('%s_%s' % (s, k), v) for s, v in p.items())
        flat = {s: v.reshape((-1,) + v.shape[(2 if k == 'members_B' else 1):]) for s, v in p.items()}
        for s in ('S', 'A', 'L'):
            res['median_%s_%s' % (s, k)] = _nan_reduce(np.nanmedian, flat[s])
        res['mean_abs_S_' + k], res['mean_abs_A_' + k] = (_nan_reduce(np.nanmean, np.abs(flat[s])) for s in ('S', 'A'))
        res['mean_L_' + k] = _nan_reduce(np.nanmean, flat['L'])
        res['defined_' + k] = (~np.isnan(flat['S']) & ~np.isnan(flat['L'])).mean(0)
    return res


MINKOWSKI_SETS = ('members_B', 'ens_mean_B', 'fake_A', 'real_B', 'real_A')
MINKOWSKI_PAIRS = (('members_B', 'real_B'), ('ens_mean_B', 'real_B'), ('fake_A', 'real_A'))


def eval_minkowski(dataset, model, n_samples, thr_B, thr_A, use_gpu=True, components=0):
    """the shape of the excursion sets on a split, one read of the counts per batch.  The counts of ops.minkowski, at the
    thresholds thr_B (C_B, T) in domain B and thr_A (C_A, T) in domain A, are summed in int64 over the fields of five sets:
    the n_samples translations A -> B of every input (members_B) and their per-pixel means (ens_mean_B)
    (model.translate_minkowski), B -> A (fake_A, predict_A), and the real fields of both domains through the same kernel
    (real_B, real_A).  Unpaired: the sets are compared as sets.  -> dict, per set k of MINKOWSKI_SETS: counts_k (C, T, 5)
    int64, cells_k int64 and the float64 (C, T) arrays of ops.minkowski_summary, area_k, perimeter_k, euler4_k, euler8_k and
    the same per cell under *_density_k; per translated set k, against the real set of its domain (MINKOWSKI_PAIRS):
    dist_area_k, dist_perimeter_k, dist_euler4_k, dist_euler8_k (C,) of ops.minkowski_distance.  components = 4 or 8: the
    connected components of the same sets under that connectivity too (ops.components, summed like the counts): per set
    comp_k (C, T, 25) int64 and the entries of ops.components_summary under <name>_k, per translated set dist_components_k,
    dist_holes_k, dist_size_k (C,) of ops.components_distance; 0: none of them, and no launch more than before"""
    sums = {k: _Sum() for k in MINKOWSKI_SETS}
    comp = {k: _Sum() for k in MINKOWSKI_SETS}
    thresholds = _domain_tables(thr_B, thr_A, check=ops.check_thresholds)
    for real_A, real_B in _batches(dataset, use_gpu):
        t_B, t_A = thresholds(real_B, real_A)
        r = model.translate_minkowski(real_A, n_samples, t_B, components=components)
        CA, CB = real_A.size(1), real_B.size(1)
        with torch.no_grad():
            pred_A = model.predict_A(real_B)
            fake_A = ops.minkowski(pred_A, CA, "nchw", t_A)
        parts = (r['members'].flatten(0, 1), r['ens_mean'], fake_A, ops.minkowski(real_B, CB, "nchw", t_B),
                 ops.minkowski(real_A, CA, "nchw", t_A))
        # the fields of a set are summed on the device: what is read is (1, C, T, 5) per set
        for k, p, v in zip(MINKOWSKI_SETS, parts, _read_back([p.sum(0, keepdim=True) for p in parts])):
            sums[k].add(v, _cells(real_A if k.endswith('_A') else real_B), rows=p.size(0))
        if components:
            parts = (r['members_comp'].flatten(0, 1), r['ens_mean_comp'], ops.components(pred_A, CA, "nchw", t_A, conn=components),
                     ops.components(real_B, CB, "nchw", t_B, conn=components), ops.components(real_A, CA, "nchw", t_A, conn=components))
            for k, p, v in zip(MINKOWSKI_SETS, parts, _read_back([p.sum(0, keepdim=True) for p in parts])):
                comp[k].add(v, rows=p.size(0))
    res, summary = {}, {}
    for k in MINKOWSKI_SETS:
        res['counts_' + k], res['cells_' + k] = np.asarray(sums[k].total, dtype=np.int64), np.int64(sums[k].cells)
        summary[k] = ops.minkowski_summary(sums[k].total, sums[k].cells)
        res.update(('%s_%s' % (name, k), v) for name, v in summary[k].items())
    for k, real in MINKOWSKI_PAIRS:
        res.update(('dist_%s_%s' % (name, k), v) for name, v in ops.minkowski_distance(summary[k], summary[real]).items())
    if components:
        for k in MINKOWSKI_SETS:
            res['comp_' + k] = np.asarray(comp[k].total, dtype=np.int64)
            summary[k] = ops.components_summary(comp[k].total, sums[k].total, sums[k].rows, sums[k].cells, components)
            res.update(('%s_%s' % (name, k), v) for name, v in summary[k].items())
        for k, real in MINKOWSKI_PAIRS:
            res.update(('%s_%s' % (name, k), v) for name, v in ops.components_distance(summary[k], summary[real]).items())
    return res


def eval_translate(dataset, model, n_samples, overlap, use_gpu=True):
    """whole-field translation of an aligned split at its stored resolution (model.translate_field, translate_field_A), one
    read per batch -> dict of float32 arrays (N, C, H, W): mean_B and std_B over the members (torch on the canvases; std
    unbiased, 0 for one member), member0_B, fake_A; and the scalars rmse_mean_B, rmse_A against the paired real fields, pooled
    over the split in float64"""
    keys = ('mean_B', 'std_B', 'member0_B', 'fake_A')
    parts = {k: [] for k in keys}
    sse, cells = np.zeros(2), np.zeros(2)
    for real_A, real_B in _batches(dataset, use_gpu):
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


# ----------------------------------------------------------------------------------------------
# The table.  A record: name; whole_field: the data is loaded UNRESIZED and the metric takes --overlap; batch_size of its dev
# and test splits; dtype: what _eval_splits casts every entry of the file to (None: as it comes);
# prepare(opt, model, arrays) -> (header, evaluate), arrays = (trainA, trainB, devA, devB, testA, testB): what is derived
# before the splits, the file's entries beside the splits' and evaluate(dataset) -> dict for _eval_splits;
# report(opt, dev, test) -> the text to print; doc: its paragraph of test.py's documentation.
# ----------------------------------------------------------------------------------------------
Metric = namedtuple('Metric', 'name whole_field batch_size dtype prepare report doc')


def _ensemble_record():
    run = {}          # prepare -> report: the model and the dev fields of the grid, which is drawn after the splits

    def prepare(opt, model, arrays):
        run.update(model=model, devA=arrays[2], devB=arrays[3])
        header = dict(n_samples=np.int64(opt.n_samples), quantiles=np.array(opt.quantiles, dtype=np.float64))
        if not int(getattr(opt, 'ens_maps', 0)):
            def scored(dataset):
                scores, hist = eval_ensemble_B(dataset, model, opt.n_samples, opt.quantiles)
                return dict(scores, rank_hist=hist)
            return header, scored
        try:
            maps = plan_ens_maps(opt, arrays)
        except ValueError as e:
            raise SystemExit(e.args[0])
        run['maps'] = [maps]                                       # then what the maps gave on dev and on test

        def scored(dataset):                                       # the same members in the same launches' order: ensemble.npz keeps its bits
            scores, hist, cells = eval_ensemble_B(dataset, model, opt.n_samples, opt.quantiles, maps=maps)
            run['maps'].append(cells)
            return dict(scores, rank_hist=hist)
        return header, scored

    def report(opt, dev, test):
        model, devA, devB = run.pop('model'), run.pop('devA'), run.pop('devB')
        vis = next(iter(AlignedIterator(devA, devB, batch_size=max(min(10, len(devA)), 1))))
        visualize_ensemble(opt, vis['A'].cuda(), vis['B'].cuda(), model, 'ensemble_0.png')
        line = ("DEV_CRPS_B: %.4f, TEST_CRPS_B: %.4f, TEST_MSE_MEAN_B: %.4f, TEST_SPREAD_B: %.4f, TEST_COVERAGE_B: %.4f"
                % (dev['crps'].mean(), test['crps'].mean(), test['mse_mean'].mean(), _pooled_spread(test['spread']),
                   test['coverage'].mean()))
        if 'maps' in run:
            maps, cells_dev, cells_test = run.pop('maps')
            arrays = dict(n_samples=np.int64(opt.n_samples), levels=np.array(maps['levels'], dtype=np.float64))
            arrays.update((k, v) for k, v in maps.items() if k != 'levels' and v is not None)
            for split, res in (('dev', cells_dev), ('test', cells_test)):
                arrays.update(('%s_%s' % (split, k), v) for k, v in res.items())
            np.savez(os.path.join(opt.res_dir, 'ensemble_maps.npz'), **arrays)
            four = lambda res: (_chan_mean(np.abs(res['bias_members_B'])), _chan_mean(res['rmse_mean_members_B']),
                                _chan_mean(res['spread_skill_members_B']),
                                _chan_mean(res['brier_members_B'][:, -1]) if 'brier_members_B' in res else float('nan'))
            line += ("\nDEV_MAP_B: %.4f %.4f %.4f %.4f, TEST_MAP_B: %.4f %.4f %.4f %.4f (domain means of |bias|, RMSE of the ensemble "
                     "mean, spread / skill, Brier score at the highest threshold)" % (four(cells_dev) + four(cells_test)))
        return line
    return Metric('ensemble', False, 200, None, prepare, report, """\
  ensemble    (new) the stochastic direction scored as a distribution: --n_samples translations A -> B of every dev and test
              input (model.translate_ensemble), per input the CRPS, its fair form, the MSE of the ensemble mean, the spread
              and the coverage of the outer --quantiles band against the paired B, and the rank histogram of B among the
              members -> <res_dir>/ensemble.npz, and grids of A, B, mean, std and the outer quantiles for the first dev batch
              of 10 (ensemble_0.png).
              --ens_maps 1 (default 0: off, ensemble.npz, ensemble_0.png and the line above as without it) draws the first
              figures of a model on a fixed grid: maps with one value per cell, taken across the inputs of the split.  Every
              cell keeps running sums over the rows of every batch (ops.cell_stats, HIP, acg_cell_stats of
              include/acgan_cell.h: doubles and exact integers added in a fixed order, the same bits whatever the layout or
              the batching), of the same members in the same group loop (model.translate_ensemble(cell_stats=...)), no random
              draw more; the state of a split stays on the device (refused above 2 GiB) and is read back once.  Pairs
              (MAP_PAIRS): members_B (the --n_samples members against the paired B; it carries the ensemble-mean and spread
              maps) and fake_A (predict_A against the paired A, one member).  Events at the quantile levels --map_quantiles
              (default 0.9,0.99; at most 8; "none": no events) of the real training fields per channel, or at
              --map_thresholds; histograms between the B - 1 quantiles k / B of the training fields, B = --map_bins (default
              32; 0: none; at most 64); quantile maps at --map_levels (default 0.5,0.95,0.99).  Per split and pair k: the raw
              state mom_k (9, C, H, W: Sx, Sxx, Sy, Syy, Sxy, S|x - y|, SS, SSy, Sw), evt_k (C, T, 4, H, W), hist_x_k,
              hist_y_k (C, B, H, W), n_k, members_k, and (ops.cell_summary, float64 on the host) mean_x_k, mean_y_k, bias_k,
              std_x_k, std_y_k, std_ratio_k, corr_k, rmse_k, mae_k, rmse_mean_k, corr_mean_k, spread_k, spread_skill_k
              (C, H, W), freq_x_k, freq_y_k, freq_bias_k, brier_k, hit_rate_k, csi_k (C, T, H, W), cdf_x_k, cdf_y_k
              (C, B - 1, H, W), ks_k, q_x_k, q_y_k (C, levels, H, W); crps_B (C, H, W), the mean of translate_ensemble's
              crps_map; with n_samples, thresholds_B, thresholds_A, edges_B, edges_A, levels -> <res_dir>/ensemble_maps.npz,
              a file of its own.  One more line is printed: the domain means of |bias|, the RMSE of the ensemble mean, spread
              / skill and the Brier score at the highest threshold, for dev and test.  1 <= H, W <= 1024""")


def _plain_prepare(eval_split, rings=False):
    """prepare of a metric that derives nothing from the training data: eval_split(dataset, model, n_samples) on each split,
    n_samples in the header (rings: and bin_counts, the cells of every ring of the square fields)"""
    def prepare(opt, model, arrays):
        header = dict(n_samples=np.int64(opt.n_samples))
        if rings:
            header['bin_counts'] = ops.spectrum_bins(arrays[2].shape[-1])
        return header, lambda d: eval_split(d, model, opt.n_samples)
    return prepare


def _spectrum_report(opt, dev, test):
    return ("DEV_LSD_B: %.4f, TEST_LSD_B: %.4f, TEST_LSD_MEAN_B: %.4f, TEST_LSD_A: %.4f"
            % (dev['lsd_B'], test['lsd_B'], test['lsd_mean_B'], test['lsd_A']))


_SPECTRUM = Metric('spectrum', False, 200, np.float64, _plain_prepare(eval_spectrum, rings=True), _spectrum_report, """\
  spectrum    (new) the variance at every spatial scale: the radially averaged power spectrum (F = fft2 of a channel, |F|^2 / S^2
              averaged over rings of integer wavenumber 0 .. S/2; a HIP FFT, ops.radial_spectrum) of --n_samples translations
              A -> B of every dev and test input and of their per-pixel mean (model.translate_spectrum) against the real B, and
              of B -> A against the real A; split-mean spectra per channel and log-spectral distances in dB over bins
              1 .. S/2 (LSD = sqrt(mean_b (10 log10(p_b / q_b))^2), spectra clamped at 1e-30, the mean over channels), computed
              on the host in float64 -> <res_dir>/spectrum.npz.  Square fields, S a power of two in 16 .. 1024.  No plot""")


def _coherence_report(opt, dev, test):
    return ("DEV_KEFF_B: %.4f, TEST_KEFF_B: %.4f, TEST_KEFF_MEAN_B: %.4f, TEST_KEFF_A: %.4f, TEST_COH_B: %.4f"
            % (dev['k_eff_members_B'].mean(), test['k_eff_members_B'].mean(), test['k_eff_ens_mean_B'].mean(),
               test['k_eff_fake_A'].mean(), test['coh_members_B'][:, 1:].mean()))


_COHERENCE = Metric('coherence', False, 200, None, _plain_prepare(eval_coherence, rings=True), _coherence_report, """\
  coherence   (new) whether that variance is in the right place: on the aligned dev and test pairs the cross-spectrum of
              prediction x and truth y per ring (Pxx, Pyy and the co-spectrum Cxy = Re(X conj Y) / S^2; ops.cross_spectrum, one
              transform for both fields) of --n_samples translations A -> B and of their per-pixel mean
              (model.translate_coherence) against the paired B, and of B -> A against the paired A.  The triples are summed
              over the split, then (ops.coherence_summary, float64 on the host) the coherence Cxy^2 / (Pxx Pyy), the signed
              correlation, the error spectrum Pxx + Pyy - 2 Cxy (the MSE split by scale) and the effective resolution k_eff:
              the first ring whose coherence falls below 0.5 (S/2 + 1: none does), printed as its mean over the channels ->
              <res_dir>/coherence.npz.  Sizes as for spectrum.  No plot""")


def _fss_record():
    sal = []          # prepare -> report, with --fss_sal: the header of sal.npz, then what eval_sal gave on dev and on test
    rel = []          # the same with --fss_rel: the header of reliability.npz, then eval_fss's second dict of dev and of test

    def _fss_prepare(opt, model, arrays):
        thr_B = fss_thresholds(arrays[1], opt.fss_quantiles, opt.fss_thresholds)     # once: dev and test share the climatology
        thr_A = fss_thresholds(arrays[0], opt.fss_quantiles, opt.fss_thresholds)
        win = tuple(opt.fss_windows)
        header = dict(n_samples=np.int64(opt.n_samples), windows=np.array(win, dtype=np.int64), thresholds_B=thr_B, thresholds_A=thr_A)
        scales = bool(getattr(opt, 'fss_scales', 0))
        if scales:                                                     # 2^j, j = 0 .. L, of the fields the splits hold
            header['scales'] = 2 ** np.arange(ops.fss_scale_levels(*np.shape(arrays[3])[-2:]), dtype=np.int64)
        evaluate = lambda d: eval_fss(d, model, opt.n_samples, thr_B, thr_A, win, scales=scales)
        if int(getattr(opt, 'fss_rel', 0)):
            rwin = ops.check_rel_windows(opt.rel_windows)
            del rel[:]
            rel.append(dict(n_samples=np.int64(opt.n_samples), windows=np.array(rwin, dtype=np.int64), thresholds_B=thr_B,
                            thresholds_A=thr_A))

            def evaluate(dataset):                                     # the same members in the same launches' order: fss.npz keeps its bits
                res, tables = eval_fss(dataset, model, opt.n_samples, thr_B, thr_A, win, scales=scales, reliability=rwin)
                rel.append(tables)
                return res
        if not int(getattr(opt, 'fss_sal', 0)):
            return header, evaluate
        del sal[:]
        explicit = getattr(opt, 'sal_thresholds', None)               # ascending, whoever built the options
        quantiles, explicit = sorted(opt.sal_quantiles), None if explicit is None else sorted(explicit)
        sal_B = fss_thresholds(arrays[1], quantiles, explicit)
        sal_A = fss_thresholds(arrays[0], quantiles, explicit)
        floor, conn = float(opt.sal_floor), int(opt.sal_conn)
        sal.append(dict(n_samples=np.int64(opt.n_samples), thresholds_B=sal_B, thresholds_A=sal_A, floor=np.float64(floor),
                        conn=np.int64(conn)))

        def with_sal(dataset):
            res = evaluate(dataset)
            dev = [torch.cuda.current_device()] if torch.cuda.is_available() else []
            with torch.random.fork_rng(devices=dev):                   # its own members; the codes of the fss entries stay what they were
                sal.append(eval_sal(dataset, model, opt.n_samples, sal_B, sal_A, floor=floor, conn=conn))
            return res
        return header, with_sal

    def _fss_report(opt, dev, test):
        levels = opt.fss_thresholds if opt.fss_thresholds is not None else opt.fss_quantiles
        t, w = int(np.argmax(levels)), len(opt.fss_windows) // 2     # the highest threshold, the median listed window
        line = ("DEV_FSS_B: %.4f, TEST_FSS_B: %.4f, TEST_FSS_PROB_B: %.4f, TEST_FSS_MEAN_B: %.4f, TEST_FSS_A: %.4f, "
                "TEST_USEFUL_SCALE_B: %.4f"
                % (_chan_mean(dev['fss_members_B'][:, t, w]), _chan_mean(test['fss_members_B'][:, t, w]),
                   _chan_mean(test['fss_ens_prob_B'][:, t, w]), _chan_mean(test['fss_ens_mean_B'][:, t, w]),
                   _chan_mean(test['fss_fake_A'][:, t, w]), float(test['useful_scale_members_B'][:, t].mean())))
        if int(getattr(opt, 'fss_scales', 0)):
            line += ("\nDEV_ISS_B: %.4f, TEST_ISS_B: %.4f, TEST_SKILL_SCALE_B: %.4f, TEST_SKILL_SCALE_PROB_B: %.4f, "
                     "TEST_SKILL_SCALE_MEAN_B: %.4f, TEST_SKILL_SCALE_A: %.4f"
                     % ((_chan_mean(dev['iss_members_B'][:, t, 0]), _chan_mean(test['iss_members_B'][:, t, 0]))
                        + tuple(float(test['skill_scale_' + k][:, t].mean()) for k in FSS_PAIRS)))
        if int(getattr(opt, 'fss_sal', 0)):
            header, sal_dev, sal_test = sal
            arrays = dict(header)
            for split, res in (('dev', sal_dev), ('test', sal_test)):
                arrays.update(('%s_%s' % (split, k), v) for k, v in res.items())
            np.savez(os.path.join(opt.res_dir, 'sal.npz'), **arrays)

            def medians(res, k):                                       # the highest threshold: the last, they are sorted
                return tuple(_chan_mean(v) for v in (res['median_S_' + k][:, -1], res['median_A_' + k], res['median_L_' + k][:, -1]))
            line += ("\nDEV_SAL_B: %.4f %.4f %.4f, TEST_SAL_B: %.4f %.4f %.4f, TEST_SAL_MEAN_B: %.4f %.4f %.4f, "
                     "TEST_SAL_A: %.4f %.4f %.4f (S, A, L)"
                     % (medians(sal_dev, 'members_B') + medians(sal_test, 'members_B') + medians(sal_test, 'ens_mean_B')
                        + medians(sal_test, 'fake_A')))
        if int(getattr(opt, 'fss_rel', 0)):
            header, rel_dev, rel_test = rel
            arrays = dict(header)
            for split, res in (('dev', rel_dev), ('test', rel_test)):
                arrays.update(('%s_%s' % (split, k), v) for k, v in res.items())
            np.savez(os.path.join(opt.res_dir, 'reliability.npz'), **arrays)
            w1 = list(header['windows']).index(1) if 1 in header['windows'] else 0
            at = lambda res, name, k: _chan_mean(res['%s_%s' % (name, k)][:, t, w1])
            three = lambda res: tuple(at(res, name, 'ens_prob_B') for name in ('bss', 'reliability', 'auc'))
            line += ("\nDEV_REL_PROB_B: %.4f %.4f %.4f, TEST_REL_PROB_B: %.4f %.4f %.4f (BSS, reliability, AUC), TEST_BSS_B: %.4f, "
                     "TEST_BSS_MEAN_B: %.4f, TEST_BSS_A: %.4f"
                     % (three(rel_dev) + three(rel_test) + tuple(at(rel_test, 'bss', k) for k in REL_PAIRS[1:])))
        return line

    return Metric('fss', False, 200, None, _fss_prepare, _fss_report, """\
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
              threshold, the mean over the channels -> <res_dir>/fss.npz.  Any H x W up to 1024.  No plot.
              --fss_scales 1 (default 0: off, file and output as without it) says at which scale the error of the same
              events sits: the intensity-scale skill score (Casati et al. 2004, Casati 2010).  The binary error field
              [x >= t] - [y >= t] (the ensemble: the exceedance probability minus [y >= t]) is split into 2-D Haar
              components on the dyadic blocks of 2^l x 2^l cells anchored at cell (0, 0), l = 0 .. L = ceil(log2(max(H, W))),
              edge blocks cut by the domain (the planes zero-padded to 2^L x 2^L; one tiling, not Casati's average over
              tilings; no bias recalibration, no dithering).  ops.fss_scales (HIP, exact) gives per level the integer triples
              (sum bf^2, sum bo^2, sum bf bo) of the blocks' event counts; summed over the split they are scale_sums_k
              (C, T, nl, 3) int64 per comparison k, and (ops.fss_scale_summary, float64) mse_scale_k (C, T, nl): the MSE of
              the component at scale 2^j, j < L, and of the mean term at j = L, which add up to the plain MSE; mse_random_k
              (C, T): the MSE of the same events placed at random; iss_k = 1 - mse_scale (L + 1) / mse_random (NaN where
              mse_random is 0; L + 1 equal shares are a convention on a padded canvas); en_rel_k: the relative difference of
              the forecast's and the truth's component energies; skill_scale_k (C, T) int64: the smallest 2^j with iss > 0
              at every mother scale from j up (2^L: none); the header gains scales = 2^j.  One more line is printed: ISS of
              members_B at the highest threshold and the finest scale on dev and test, and the test skill scales of
              members_B, ens_prob_B, ens_mean_B and fake_A, channel means.
              --fss_sal 1 (default 0: off, fss.npz and the output as without it) adds the object-based partner of the FSS,
              the SAL score (Wernli et al. 2008): what a forecaster asks first of a paired translation, object by object.
              The objects of a field are the connected components (--sal_conn 4 | 8, default 8) of its excursion set
              {x >= t}; thresholds: per channel the --sal_quantiles (default 0.9) of the real training fields (trainB for
              A -> B, trainA for B -> A; fss_thresholds), or the --sal_thresholds in data units, sorted ascending.  The mass of
              a cell is its amount above --sal_floor (default -1, the lower end of the data range) as the fixed-point integer
              q = clamp(rint((x - floor) 2^20), 0, 2^24), so every sum is exact; ops.sal (HIP: the union-find forest of
              ops.components with the mass, the peak and the centre of mass reduced per object) gives per field Q, QY, QX and
              per threshold n, area, Robj, Rmax and the double sums SV = sum R (R / P), SR = sum R |c_object - c_field|.  Per
              PAIR (ops.sal_scores, float64 on the host): A = (Q_f - Q_o) / (0.5 (Q_f + Q_o)), the amplitude: too much or too
              little overall; S = (V_f - V_o) / (0.5 (V_f + V_o)), V = SV / Robj, the structure: > 0 for objects too large
              or too flat, < 0 for too small or too peaked; L = L1 + L2, the location: the distance of the centres of mass
              and the difference of the objects' spread about them, over the diagonal.  S, A in [-2, 2], L in [0, 2]; S and
              L are NaN where either side has no mass above the threshold.  Compared on the same aligned pairs, with members
              of its own (model.translate_sal; a forked generator, so the codes of the fss entries stay what they were):
              members_B and ens_mean_B against the paired B, fake_A against the paired A.  Per comparison k: S_k, L2_k, L_k
              (N, [M,] C, T), A_k, L1_k (N, [M,] C) per input; median_S_k, median_A_k, median_L_k (NaN-aware), mean_abs_S_k,
              mean_abs_A_k, mean_L_k and defined_k, the fraction of pairs whose S and L exist, with n_samples, thresholds_B,
              thresholds_A, floor, conn -> <res_dir>/sal.npz, a file of its own.  The mean of an ensemble is smoother than
              its members: a positive S.  One more line is printed: the medians of S, A and L at the highest threshold, the
              channel means, for the members on dev and test, the ensemble mean and B -> A.  1 <= H, W <= 1024.
              --fss_rel 1 (default 0: off, fss.npz and the lines before as without it) asks what a forecaster asks first of
              the ensemble as a probability: when k of the M = --n_samples members say "event", how often does it happen
              (Murphy 1973)?  Per channel, threshold (those of the fss entries) and odd window n of --rel_windows (default
              1,5,17; at most 8, each at most 65) the neighbourhood event of a cell is any event inside the centred n x n
              window (the neighbourhood maximum ensemble probability, Schwartz & Sobash 2017; n = 1: the cell), and
              ops.reliability (HIP, exact; acg_reliability of include/acgan_verif.h) counts the cells by k and by the truth's
              neighbourhood event: table[k][o], (M + 1, 2) int64, every table summing to H W.  The same members in the same
              group loop (model.translate_fss(reliability=...)), no random draw more.  Comparisons (REL_PAIRS): ens_prob_B
              (M + 1 forecast values k / M), every single member (members_B), the ensemble mean (ens_mean_B) and B -> A
              (fake_A: predict_A against the paired A at thresholds_A), the last three as 2 x 2 contingency tables.  Summed
              over the split, then (ops.reliability_summary, float64 on the host) per comparison k: table_k, n_k, prob_k,
              obs_freq_k (the reliability diagram; n_k is its sharpness histogram), base_rate_k, brier_k and its
              decomposition reliability_k - resolution_k + uncertainty_k (exact: nothing is binned), bss_k = 1 - brier /
              uncertainty, brier_fair_k (Ferro 2014: what infinitely many members would score; NaN for one), roc_hit_k,
              roc_false_k (M + 2 points) and auc_k (trapezoid; the Mann-Whitney statistic), with n_samples, windows,
              thresholds_B, thresholds_A -> <res_dir>/reliability.npz, a file of its own.  One more line is printed: the
              Brier skill score, the reliability term and the AUC of ens_prob_B at the highest threshold and window 1 (the
              first listed if 1 is absent) on dev and test, then the test BSS of a single member, of the ensemble mean and
              of B -> A, channel means""")


def _translate_record():
    rmse = []         # evaluate -> report: the file holds the maps; the two scalars of each split are only printed

    def prepare(opt, model, arrays):
        devA = arrays[2]
        plan = ops.window_plan(devA.shape[2], devA.shape[3], opt.grid_size, opt.overlap)
        header = dict(n_samples=np.int64(opt.n_samples), window=np.int64(opt.grid_size), overlap=np.int64(opt.overlap),
                      origins_y=np.array(plan.oy[:plan.ny], dtype=np.int64), origins_x=np.array(plan.ox[:plan.nx], dtype=np.int64))
        del rmse[:]

        def translated(dataset):
            res = eval_translate(dataset, model, opt.n_samples, opt.overlap)
            rmse.append((res.pop('rmse_mean_B'), res.pop('rmse_A')))
            return res
        return header, translated

    def report(opt, dev, test):
        return "DEV_RMSE_MEAN_B: %.4f, TEST_RMSE_MEAN_B: %.4f, TEST_RMSE_A: %.4f" % (rmse[0][0], rmse[1][0], rmse[1][1])
    # batches of at most 8 fields: a batch's canvases of every member stay on the device until they are read
    return Metric('translate', True, 8, np.float32, prepare, report, """\
  translate   (new) whole fields at their stored resolution: the data is loaded UNRESIZED, every dev and test field of any
              H x W >= grid_size is cut into overlapping grid_size windows (--overlap pixels shared by neighbours, default
              grid_size // 4), translated window by window and blended at the seams (model.translate_field, --n_samples
              members per field with one code each; model.translate_field_A for B -> A).  Per split, float32:
              <split>_mean_B, <split>_std_B (over the members, unbiased; 0 for one member), <split>_member0_B and
              <split>_fake_A, each (N, C, H, W), with n_samples, window, overlap, origins_y, origins_x ->
              <res_dir>/translate.npz.  Printed: the RMSE of the member mean against the paired B and of fake_A against the
              paired A.  No plot""")


def _field_spectrum_prepare(opt, model, arrays):
    devA = arrays[2]
    header = dict(n_samples=np.int64(opt.n_samples), window=np.int64(opt.grid_size), overlap=np.int64(opt.overlap),
                  height=np.int64(devA.shape[2]), width=np.int64(devA.shape[3]))
    return header, lambda d: eval_field_spectrum(d, model, opt.n_samples, opt.overlap)


def _field_spectrum_report(opt, dev, test):
    return ("DEV_LSD_B: %.4f, TEST_LSD_B: %.4f, DEV_LSD_A: %.4f, TEST_LSD_A: %.4f, DEV_K_EFF_B: %.4f, TEST_K_EFF_B: %.4f"
            % (dev['lsd_B'], test['lsd_B'], dev['lsd_A'], test['lsd_A'], dev['k_eff_members_B'].mean(),
               test['k_eff_members_B'].mean()))


# batches of 8, as translate: whole canvases of every member
_FIELD_SPECTRUM = Metric('field_spectrum', True, 8, None, _field_spectrum_prepare, _field_spectrum_report, """\
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
              of the members.  No plot""")


def _ssim_report(opt, dev, test):
    return ("DEV_SSIM_B: %.4f, TEST_SSIM_B: %.4f, TEST_CS_B: %.4f, TEST_SSIM_MEAN_B: %.4f, TEST_CS_MEAN_B: %.4f, "
            "TEST_SSIM_A: %.4f, TEST_CS_A: %.4f"
            % (dev['ssim_members_B'].mean(), test['ssim_members_B'].mean(), test['cs_members_B'].mean(),
               test['ssim_ens_mean_B'].mean(), test['cs_ens_mean_B'].mean(), test['ssim_fake_A'].mean(),
               test['cs_fake_A'].mean()))


_SSIM = Metric('ssim', False, 200, np.float64, _plain_prepare(eval_ssim), _ssim_report, """\
  ssim        (new) the local structure: the structural similarity (Wang et al. 2004; 11 x 11 Gaussian window, sigma 1.5,
              data range 2, valid positions; ops.ssim, HIP) on the aligned dev and test pairs, of the --n_samples translations
              A -> B (members_B) and of their per-pixel mean (ens_mean_B) (model.translate_ssim) against the paired B, and
              of B -> A (fake_A) against the paired A.  Per comparison k, float64: ssim_k and cs_k (C,), the split means of
              the mean S and of the mean contrast-structure factor cs, and ssim_k_per_input, cs_k_per_input (N, C), the
              members averaged per input -> <res_dir>/ssim.npz.  The mean of an ensemble is smoother than its members: a
              higher luminance term, a lower cs; the file shows both.  Printed: the channel means.  11 <= H, W <= 1024.
              No plot""")


def _marginal_prepare(opt, model, arrays):
    edges_B = marginal_edges(arrays[1], opt.marg_bins)            # once: dev and test share the climatology
    edges_A = marginal_edges(arrays[0], opt.marg_bins)
    levels = tuple(opt.marg_levels)
    header = dict(n_samples=np.int64(opt.n_samples), levels=np.array(levels, dtype=np.float64), edges_B=edges_B, edges_A=edges_A)
    return header, lambda d: eval_marginal(d, model, opt.n_samples, levels, edges_B, edges_A)


def _marginal_report(opt, dev, test):
    return ("DEV_W1_B: %.4f, TEST_W1_B: %.4f, TEST_W1_MEAN_B: %.4f, TEST_W1_A: %.4f, TEST_KS_B: %.4f, TEST_KS_MEAN_B: %.4f, "
            "TEST_KS_A: %.4f"
            % (dev['w1_members_B'].mean(), test['w1_members_B'].mean(), test['w1_ens_mean_B'].mean(), test['w1_fake_A'].mean(),
               test['ks_members_B'].mean(), test['ks_ens_mean_B'].mean(), test['ks_fake_A'].mean()))


_MARGINAL = Metric('marginal', False, 200, None, _marginal_prepare, _marginal_report, """\
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
              Printed: the channel means of w1 and ks.  H W <= 2^20.  No plot""")


def _minkowski_prepare(opt, model, arrays):
    thr_B = marginal_edges(arrays[1], opt.mink_bins)              # once: dev and test share the climatology
    thr_A = marginal_edges(arrays[0], opt.mink_bins)
    header = dict(n_samples=np.int64(opt.n_samples), bins=np.int64(opt.mink_bins), thresholds_B=thr_B, thresholds_A=thr_A)
    conn = int(getattr(opt, 'mink_components', 0))
    if conn:
        header['connectivity'] = np.int64(conn)
    return header, lambda d: eval_minkowski(d, model, opt.n_samples, thr_B, thr_A, components=conn)


def _minkowski_report(opt, dev, test):
    lines = ["%s_MINK_B: %s, %s_MINK_MEAN_B: %s, %s_MINK_A: %s (area, perimeter, euler4, euler8)"
             % tuple(v for k in ('members_B', 'ens_mean_B', 'fake_A')
                     for v in (name, " ".join("%.6f" % _chan_mean(res['dist_%s_%s' % (f, k)]) for f in ops.MINK_FUNCTIONALS)))
             for name, res in (('DEV', dev), ('TEST', test))]
    if int(getattr(opt, 'mink_components', 0)):
        lines += ["%s_COMP_B: %s, %s_COMP_MEAN_B: %s, %s_COMP_A: %s (components, holes, size; %d-connected)"
                  % (tuple(v for k in ('members_B', 'ens_mean_B', 'fake_A')
                           for v in (name, " ".join("%.6f" % _chan_mean(res['dist_%s_%s' % (f, k)]) for f in ('components', 'holes', 'size'))))
                     + (int(opt.mink_components),))
                  for name, res in (('DEV', dev), ('TEST', test))]
    return "\n".join(lines)


_MINKOWSKI = Metric('minkowski', False, 200, None, _minkowski_prepare, _minkowski_report, """\
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
              four distances of members_B, ens_mean_B and fake_A, the channel means.  1 <= H, W <= 1024.  No plot.
              --mink_components 4 | 8 (default 0: off, file and output as without it) labels the connected components of
              the same sets under that connectivity (ops.components, HIP union-find, exact integers) - the Euler numbers only
              give components MINUS holes - and adds, per set k: comp_k (C, T, 25) int64 = n, area, sum of squared areas,
              n_border and the 21 bins of floor(log2(area)) summed over the fields, and (ops.components_summary) components_k,
              holes_k = components - euler, both per cell (*_density_k), mean_area_k, weighted_area_k, border_fraction_k
              (C, T) and size_pdf_k (C, T, 21); per translated set (ops.components_distance) dist_components_k, dist_holes_k
              and dist_size_k (C,), the total-variation distance of the size distributions; connectivity in the header; one
              more printed line per split: the three distances, the channel means""")


METRICS = (_ensemble_record(), _SPECTRUM, _COHERENCE, _fss_record(), _translate_record(), _FIELD_SPECTRUM, _SSIM, _MARGINAL, _MINKOWSKI)
WHOLE_FIELD_METRICS = tuple(m.name for m in METRICS if m.whole_field)
