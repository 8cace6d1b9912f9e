"""Dataset calibration (the reference's calibration/extract_features.py, train.py and data.py; calibration/README.md): fit the model's
parameters to a table of subjective scores.

    python -m colorvideovdp_amd.calibration extract quality.csv -d standard_4k
    python -m colorvideovdp_amd.calibration fit quality.csv -o new_config

`extract` scores every row of the quality file once and writes its Q_per_ch as `features[_suffix]/{train,test}/<id>_fmap.json`
(cvvdp.write_features_to_json).  `fit` loads those files into a FeatureSet -- all clips packed into one device buffer -- and runs Adam on
the mean squared error of the JOD over the pooling parameters: every step is one launch of cvvdp_pool_dataset (the JOD of every clip of
the mini-batch and its gradient in the nine pooling parameters, csrc/pool_dataset.hip) and one of cvvdp_pool_dataset_loss, with the
parameters, their gradient and the optimiser's state on the device.  Naming a band parameter (cvvdp_metric.BAND_PARAMETERS) in
`--parameters` switches `fit` to rescoring mode: the clips are scored again on every step with
predict_video_source_with_parameter_gradient(), which is the full fit the reference ships no script for.

`-m cvvdp-ml-saliency` calibrates the ML head instead: `extract` writes the per-cell features of every row as
`<id>_mlfeat.npz`, and `fit` runs Adam on the packed weights of both MLPs (and on the model's scalar baseband_weight when `--parameters
baseband_weight` names it) through cvvdp_ml_saliency.differentiable_jods, whose backward is cvvdp_ml_saliency_head_grad.  It writes
OUT/cvvdp_ml_saliency/cvvdp.ckpt and cvvdp_parameters.json, which cvvdp_ml_saliency(config_paths=[OUT]) loads.  Deviation D2 from the
reference's training: no dropout (its MLPs carry Dropout(0.2) in training mode); the fit is deterministic.

Only the standard library, numpy and torch are used.  Deviation D1 from train.py: the mini-batch order is
numpy.random.default_rng(seed + epoch).permutation, not the DataLoader's; with -b at or above the size of the training set the two
agree up to the order of summation.  DESIGN.md 7j has the layout, the summation order and what stays out."""
import argparse
import csv
import ctypes
import json
import logging
import os
import re
import sys
import time

import numpy as np
import torch

from . import _capi
from .cvvdp_metric import BAND_PARAMETERS, POOLING_PARAMETERS
from .vq_metric import vq_exception

# theta of cvvdp_pool_dataset: name -> slots of the nine doubles
THETA_SLOTS = {"ch_chrom_w": (0, 1), "ch_trans_w": (1, 2), "baseband_weight": (2, 6), "jod_a": (6, 7), "jod_exp": (7, 8), "image_int": (8, 9)}
THETA_COUNT = _capi.POOL_THETA_COUNT
DEFAULT_PARAMETERS = ("ch_chrom_w", "ch_trans_w", "baseband_weight", "jod_a", "jod_exp")      # train.py:71, 75
BAND_COUNT = _capi.PARAM_GRAD_COUNT
assert tuple(THETA_SLOTS) == POOLING_PARAMETERS


# ---------------------------------------------------------------- the quality file
def read_quality_file(path):
    """(header, columns, rows) of a quality file.  The header (extract_features.py:11-38) is the run of lines before the table: blank
    lines and lines starting with `#` are skipped, a line `key: value` is an option, and the first other line without a `:` starts the
    table.  header: list of (key with - as _, value); rows: one dict per table row, every value a string."""
    if not os.path.isfile(path):
        raise vq_exception(f"Quality file not found at: {path}")
    with open(path, newline="") as f:
        lines = f.read().splitlines()
    header, n = [], 0
    for line in lines:
        line = line.strip("\n ")
        if line == "" or line.startswith("#"):
            n += 1
            continue
        if ":" not in line:
            break
        pos = line.find(":")
        header.append((line[:pos].replace("-", "_"), line[pos + 1:].strip()))
        n += 1
    reader = csv.DictReader([l for l in lines[n:] if l.strip() != ""], skipinitialspace=True)
    columns = [c.strip() for c in (reader.fieldnames or [])]
    reader.fieldnames = columns
    rows = [{k: (v.strip() if isinstance(v, str) else v) for k, v in r.items()} for r in reader]
    for need in ("test", "reference"):
        if need not in columns:
            raise vq_exception(f"'{path}': the table has no column '{need}' (columns: {', '.join(columns)})")
    return header, columns, rows


def header_arguments(header, known):
    """The header's options as command-line words, to be put BEHIND the command line so that they override it (extract_features.py:29-33):
    `key: true` is a flag, anything else `--key value`.  Keys the parser does not know are skipped with a warning."""
    words = []
    for key, val in header:
        if key not in known:
            logging.warning(f"{key} not found in argparse namespace, skipping")
            continue
        flag = "--" + key.replace("_", "-")
        words += [flag] if val.lower() == "true" else [flag, val]
    return words


def row_id(test):
    """The unique id of a row: the test path without its extension, `/` as `_` (extract_features.py:122)."""
    return os.path.splitext(test)[0].replace("/", "_")


def split_conditions(values, seed, train_ratio):
    """train.py:80-82: the unique values of the split column in order of first appearance, permuted by numpy's legacy generator seeded
    with `seed` (the stream numpy.random.seed(seed) sets up, without touching the global state); the first len * ratio // 100 are the
    training conditions.  Returns (train conditions, all conditions permuted)."""
    unique = list(dict.fromkeys(values))
    arr = np.empty(len(unique), dtype=object)
    arr[:] = unique
    perm = np.random.RandomState(seed).permutation(arr)
    return list(perm[:(len(perm) * int(train_ratio)) // 100]), list(perm)


def split_rows(rows, column, seed, train_ratio):
    """(train rows, test rows), train.py:83-84."""
    if not rows or column not in rows[0]:
        raise vq_exception(f'Split column "{column}" not found')
    train_cond = set(split_conditions([r[column] for r in rows], seed, train_ratio)[0])
    return [r for r in rows if r[column] in train_cond], [r for r in rows if r[column] not in train_cond]


def features_dir(suffix):
    return "features" if suffix is None else "features_" + suffix


# ---------------------------------------------------------------- validation measures
def average_ranks(x):
    """Ranks 1..n of x, ties sharing the mean of their ranks (float64)."""
    x = np.asarray(x, dtype=np.float64)
    order = np.argsort(x, kind="stable")
    ranks = np.empty(len(x), dtype=np.float64)
    sx = x[order]
    i = 0
    while i < len(x):
        j = i
        while j + 1 < len(x) and sx[j + 1] == sx[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    return ranks


def pearson(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    xm, ym = x - x.mean(), y - y.mean()
    den = np.sqrt((xm * xm).sum() * (ym * ym).sum())
    return float((xm * ym).sum() / den) if den > 0 else float("nan")


def measures(predicted, target):
    """RMSE, Pearson and Spearman (average ranks for ties) of two vectors, float64."""
    p, t = np.asarray(predicted, dtype=np.float64).reshape(-1), np.asarray(target, dtype=np.float64).reshape(-1)
    if p.shape != t.shape or p.size < 1:
        raise vq_exception("measures: two vectors of the same, non-zero length are needed")
    return {"rmse": float(np.sqrt(np.mean((p - t) ** 2))), "pearson": pearson(p, t), "spearman": pearson(average_ranks(p), average_ranks(t))}


# ---------------------------------------------------------------- the packed set
def clips_of_feature_file(fname):
    """The float32 [C][F][L] arrays of a file cvvdp.write_features_to_json wrote, one per batch item (data.py:43-65)."""
    with open(fname, "r", encoding="utf-8") as f:
        fmap = json.load(f)
    keys = [k for k in fmap if re.fullmatch(r"t\d+_b\d+", k)]
    if not keys:
        raise vq_exception(f"'{fname}' holds no t<channel>_b<band> entries")
    C = 1 + max(int(k.split("_")[0][1:]) for k in keys)
    L = 1 + max(int(k.split("_")[1][1:]) for k in keys)
    if len(keys) != C * L:
        raise vq_exception(f"'{fname}': {len(keys)} t<channel>_b<band> entries, expected {C} x {L}")
    B, F = len(fmap["t0_b0"]), len(fmap["t0_b0"][0])
    q = np.empty((B, C, F, L), dtype=np.float32)
    for c in range(C):
        for b in range(L):
            v = np.asarray(fmap[f"t{c}_b{b}"], dtype=np.float32)
            if v.shape != (B, F):
                raise vq_exception(f"'{fname}': t{c}_b{b} has shape {v.shape}, expected {(B, F)}")
            q[:, c, :, b] = v
    return [q[i] for i in range(B)]


class FeatureSet:
    """A ragged set of clips' Q_per_ch, packed once: one float32 buffer, the clips' offsets and shapes, and optionally their target JODs.
    Packing and every check happen on the host; the arrays go to the device at the first use and stay there.

    clips: arrays or tensors [C][F][L] (anything numpy reads; stored as float32).  C in 1..4, L in 1..16, F >= 1."""

    def __init__(self, clips, targets=None, device=None, ids=None):
        clips = [np.ascontiguousarray(c.detach().cpu().numpy() if torch.is_tensor(c) else c, dtype=np.float32) for c in clips]
        if not clips:
            raise vq_exception("FeatureSet: no clips")
        for i, c in enumerate(clips):
            if c.ndim != 3:
                raise vq_exception(f"FeatureSet: clip {i} has {c.ndim} dimensions, expected [C][F][L]")
            C, F, L = c.shape
            if not 1 <= C <= 4:
                raise vq_exception(f"FeatureSet: clip {i} has {C} channels, expected 1 to 4")
            if not 1 <= L <= _capi.MAX_LEVELS:
                raise vq_exception(f"FeatureSet: clip {i} has {L} bands, expected 1 to {_capi.MAX_LEVELS}")
            if F < 1:
                raise vq_exception(f"FeatureSet: clip {i} has no frames")
        self.clips = clips
        self.shapes = np.asarray([c.shape for c in clips], dtype=np.int32).reshape(-1, 3)
        sizes = self.shapes.astype(np.int64).prod(axis=1)
        self.offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        self.packed = np.concatenate([c.reshape(-1) for c in clips])
        if np.any(self.offsets + sizes > self.packed.size):
            raise vq_exception("FeatureSet: a clip lies outside the packed buffer")
        self.ids = list(ids) if ids is not None else None
        self.targets = None
        if targets is not None:
            self.targets = np.asarray(targets, dtype=np.float64).reshape(-1)
            if self.targets.size != len(clips):
                raise vq_exception(f"FeatureSet: {self.targets.size} targets for {len(clips)} clips")
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self._dev = None
        self._handle = None

    def __len__(self):
        return len(self.clips)

    def __del__(self):
        try:
            if getattr(self, "_handle", None) is not None and self._handle.value:
                _capi.lib().cvvdp_destroy(self._handle)
                self._handle = None
        except Exception:
            pass

    @classmethod
    def from_stats(cls, stats_list, targets=None, device=None, ids=None):
        """From the `stats` dicts of predict_video_source() (or bare Q_per_ch [B][C][F][L]): one clip per batch item, a target per clip."""
        clips = []
        for s in stats_list:
            q = s["Q_per_ch"] if isinstance(s, dict) else s
            q = q.detach().cpu().numpy() if torch.is_tensor(q) else np.asarray(q)
            if q.ndim != 4:
                raise vq_exception(f"FeatureSet: Q_per_ch has {q.ndim} dimensions, expected [B][C][F][L]")
            clips += [q[b] for b in range(q.shape[0])]
        return cls(clips, targets, device, ids)

    @classmethod
    def from_files(cls, fnames, targets=None, device=None, ids=None):
        """From feature files, one target per file; a file with several batch items gives several clips with the file's target."""
        clips, tg = [], []
        for i, fname in enumerate(fnames):
            if not os.path.isfile(fname):
                raise vq_exception(f'Features missing: "{fname}" (run `extract` first)')
            got = clips_of_feature_file(fname)
            clips += got
            if targets is not None:
                tg += [targets[i]] * len(got)
        return cls(clips, tg if targets is not None else None, device, ids)

    def on_device(self):
        """The device arrays (made once): q, offset, shape, target (or None), and the handle that carries the error text."""
        if self._dev is None:
            if not torch.cuda.is_available():
                raise RuntimeError("no HIP device available: colorvideovdp_amd has no CPU path")
            dev = self.device
            d = {"q": torch.from_numpy(self.packed).to(dev), "offset": torch.from_numpy(self.offsets).to(dev),
                 "shape": torch.from_numpy(self.shapes).to(dev).contiguous(),
                 "target": torch.from_numpy(self.targets).to(dev) if self.targets is not None else None}
            params = _capi.Params()
            params.blur_radius = 6
            h = ctypes.c_void_p()
            rc = _capi.lib().cvvdp_create(ctypes.byref(params), ctypes.byref(h))
            if rc != 0:
                raise RuntimeError(f"cvvdp_create failed ({rc})")
            self._handle, self._dev = h, d
        return self._dev

    def check_index(self, index):
        """A mini-batch's clip numbers as a host int32 array, each inside the set."""
        idx = np.asarray(index.detach().cpu().numpy() if torch.is_tensor(index) else index)
        if idx.ndim != 1 or idx.size < 1 or idx.dtype.kind not in "iu":
            raise vq_exception("pool_dataset: index must be a non-empty vector of integers")
        if idx.min() < 0 or idx.max() >= len(self):
            raise vq_exception(f"pool_dataset: index outside 0 .. {len(self) - 1}")
        return idx.astype(np.int32)

    def _pool(self, theta, betas, index_dev, n, jod=None, grad=None):
        """One launch of cvvdp_pool_dataset; index_dev: int32 device tensor already checked, or None."""
        d = self.on_device()
        dev = self.device
        if jod is None:
            jod = torch.empty((n,), dtype=torch.float64, device=dev)
            grad = torch.empty((n, THETA_COUNT), dtype=torch.float64, device=dev)
        b = (ctypes.c_double * 3)(*[float(x) for x in betas])
        rc = _capi.lib().cvvdp_pool_dataset(self._handle, d["q"].data_ptr(), d["offset"].data_ptr(), d["shape"].data_ptr(),
                                            index_dev.data_ptr() if index_dev is not None else None, n, theta.data_ptr(), b,
                                            jod.data_ptr(), grad.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        _capi.check(self._handle, rc, "cvvdp_pool_dataset")
        return jod, grad

    def _loss(self, jod, grad, target, n, loss=None, dloss=None):
        dev = self.device
        if loss is None:
            loss = torch.empty((1,), dtype=torch.float64, device=dev)
        if dloss is None:
            dloss = torch.empty((THETA_COUNT,), dtype=torch.float64, device=dev)
        rc = _capi.lib().cvvdp_pool_dataset_loss(self._handle, jod.data_ptr(), grad.data_ptr(), target.data_ptr(), n, loss.data_ptr(),
                                                 dloss.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        _capi.check(self._handle, rc, "cvvdp_pool_dataset_loss")
        return loss, dloss


def _theta_tensor(theta, device):
    if torch.is_tensor(theta):
        t = theta.detach()
        if t.dtype != torch.float64 or t.numel() != THETA_COUNT:
            raise vq_exception(f"pool_dataset: theta must hold {THETA_COUNT} float64 values")
        return t.to(device).contiguous()
    t = np.asarray(theta, dtype=np.float64).reshape(-1)
    if t.size != THETA_COUNT:
        raise vq_exception(f"pool_dataset: theta must hold {THETA_COUNT} values")
    return torch.from_numpy(t).to(device)


def _betas(betas):
    b = [float(x) for x in betas]
    if len(b) != 3 or not all(x > 0 and np.isfinite(x) for x in b):
        raise vq_exception("pool_dataset: betas must be three positive numbers (beta_sch, beta_tch, beta_t)")
    return b


def pool_dataset(features, theta, betas, index=None):
    """(jod [n], grad [n][9]) as float64 device tensors: the JOD of the clips `index` of `features` (None: all, in order) and its gradient
    in theta = (ch_chrom_w, ch_trans_w, baseband_weight[0..3], jod_a, jod_exp, image_int), a sequence or a float64 tensor (on the device:
    no copy).  betas = (beta_sch, beta_tch, beta_t).  One launch; row i is clip index[i], bit for bit what it is in any other call."""
    b = _betas(betas)
    idx = features.check_index(index) if index is not None else None
    if (torch.is_tensor(theta) and theta.numel() != THETA_COUNT) or (not torch.is_tensor(theta) and np.size(theta) != THETA_COUNT):
        raise vq_exception(f"pool_dataset: theta must hold {THETA_COUNT} values")
    features.on_device()
    th = _theta_tensor(theta, features.device)
    index_dev = torch.from_numpy(idx).to(features.device) if idx is not None else None
    return features._pool(th, b, index_dev, len(idx) if idx is not None else len(features))


def dataset_loss(features, jod, grad, target=None):
    """(loss [1], dloss [9]), float64 on the device: mean squared error of jod against target (None: the set's own targets, for a call
    over the whole set) and its gradient (2/n) sum (jod - target) grad, by cvvdp_pool_dataset_loss."""
    d = features.on_device()
    target = d["target"] if target is None else target
    if target is None:
        raise vq_exception("dataset_loss: the set has no targets")
    n = int(jod.numel())
    if target.numel() != n or grad.numel() != n * THETA_COUNT or jod.dtype != torch.float64 or grad.dtype != torch.float64 or target.dtype != torch.float64:
        raise vq_exception("dataset_loss: jod [n], grad [n][9] and target [n] must be float64 and agree in n")
    return features._loss(jod.contiguous(), grad.contiguous(), target.contiguous(), n)


def theta_of(parameters):
    """The nine pooling values of a parameter dictionary as the metric holds them (float32), in float64."""
    t = np.zeros(THETA_COUNT, dtype=np.float64)
    for name, (a, b) in THETA_SLOTS.items():
        t[a:b] = np.asarray(parameters[name], dtype=np.float32).reshape(-1)
    return t


def betas_of(parameters):
    return [float(np.float32(parameters[n])) for n in ("beta_sch", "beta_tch", "beta_t")]


def parameter_names(names):
    """--parameters checked: (pooling names, band names)."""
    names = list(DEFAULT_PARAMETERS if names is None else names)
    for n in names:
        if n not in THETA_SLOTS and n not in BAND_PARAMETERS:
            raise vq_exception(f"unknown parameter '{n}': calibration fits {', '.join(list(THETA_SLOTS) + list(BAND_PARAMETERS))}")
    if not names:
        raise vq_exception("no parameter to fit")
    return [n for n in names if n in THETA_SLOTS], [n for n in names if n in BAND_PARAMETERS]


def _mask(names, slots, count):
    m = np.zeros(count, dtype=np.float64)
    for n in names:
        a, b = slots[n]
        m[a:b] = 1.0
    return m


class _Log:
    """`-l DIR`: DIR/log.csv in place of tensorboard, one line per step for the loss and one per validation."""

    def __init__(self, log_dir):
        self.f = None
        if log_dir:
            os.makedirs(log_dir, exist_ok=True)
            self.f = open(os.path.join(log_dir, "log.csv"), "w", newline="")
            self.w = csv.writer(self.f)
            self.w.writerow(["kind", "epoch", "step", "loss", "rmse", "pearson", "spearman"])

    def loss(self, epoch, step, value):
        if self.f:
            self.w.writerow(["train", epoch, step, repr(float(value)), "", "", ""])

    def validation(self, epoch, score):
        if self.f:
            self.w.writerow(["val", epoch, "", "", repr(score["rmse"]), repr(score["pearson"]), repr(score["spearman"])])

    def close(self):
        if self.f:
            self.f.close()
            self.f = None


class _Keeper:
    """--save: which parameters are written at the end (train.py:98-102, 124-129, 161-162)."""

    def __init__(self, save):
        if save not in ("latest", "best-rmse", "best-pearson", "best-spearman"):
            raise vq_exception(f"--save {save}: one of latest, best-rmse, best-pearson, best-spearman")
        self.monitor = save.split("-")[1] if save.startswith("best") else None
        self.score = float("inf") if self.monitor == "rmse" else -float("inf")
        self.epoch, self.state = -1, None

    def offer(self, epoch, score, state):
        if self.monitor is None:
            return
        s = score[self.monitor]
        if (self.monitor == "rmse" and s < self.score) or (self.monitor != "rmse" and s > self.score):
            self.score, self.epoch, self.state = s, epoch, state()


def _batches(n, batch, seed, epoch):
    perm = np.random.default_rng(seed + epoch).permutation(n).astype(np.int32)          # D1
    return perm, [(a, min(a + batch, n)) for a in range(0, n, batch)]


def fit_features(train, val, parameters, names=None, batch=4, learning_rate=1e-3, num_epochs=50, val_epoch=1, save="latest", seed=0,
                 log_dir=None, steps=None):
    """Adam on the mean squared error of the JOD over the pooling parameters `names`, on packed features (train.py:131-156).
    train, val: FeatureSet with targets (val may be None); parameters: the metric's parameter dictionary (start values, betas).
    One float64 device tensor of nine entries is optimised; its .grad is the output of cvvdp_pool_dataset_loss with the entries that are
    not fitted masked to 0.  steps: stop after this many optimiser steps (tests).  Returns a dict: theta (the parameters to store, per
    --save), epoch, theta_latest, losses (one per step), validation (list of (epoch, measures))."""
    pool_names, band_names = parameter_names(names)
    if band_names:
        raise vq_exception("fit_features: band parameters need rescoring mode (fit_rescoring)")
    if train.targets is None or (val is not None and val.targets is None):
        raise vq_exception("fit: the feature sets need targets")
    if batch < 1 or num_epochs < 0 or val_epoch < 1:
        raise vq_exception("fit: batch and val-epoch must be at least 1, num-epochs at least 0")
    keeper = _Keeper(save)
    betas = _betas(betas_of(parameters))
    dev = train.device
    d = train.on_device()
    theta = torch.from_numpy(theta_of(parameters)).to(dev).requires_grad_(True)
    theta.grad = torch.zeros_like(theta)
    mask = torch.from_numpy(_mask(pool_names, THETA_SLOTS, THETA_COUNT)).to(dev)
    opt = torch.optim.Adam([theta], lr=learning_rate)
    n = len(train)
    nb = min(batch, n)
    jod = torch.empty((nb,), dtype=torch.float64, device=dev)
    grad = torch.empty((nb, THETA_COUNT), dtype=torch.float64, device=dev)
    dloss = torch.empty((THETA_COUNT,), dtype=torch.float64, device=dev)
    log = _Log(log_dir)
    losses, validation = [], []

    def validate(epoch):
        if val is None:
            return
        j, _ = val._pool(theta.detach(), betas, None, len(val))
        score = measures(j.cpu().numpy(), val.targets)
        validation.append((epoch, score))
        log.validation(epoch, score)
        logging.info(f"epoch {epoch}: validation rmse {score['rmse']:.4f} pearson {score['pearson']:.4f} spearman {score['spearman']:.4f}")
        keeper.offer(epoch, score, lambda: theta.detach().cpu().numpy().copy())

    try:
        validate(-1)
        done, epoch = 0, -1
        for epoch in range(num_epochs):
            perm, cuts = _batches(n, batch, seed, epoch)
            perm_dev = torch.from_numpy(perm).to(dev)
            target_dev = d["target"][perm_dev.long()]
            step_loss = torch.empty((len(cuts),), dtype=torch.float64, device=dev)
            for i, (a, b) in enumerate(cuts):
                train._pool(theta.detach(), betas, perm_dev[a:b], b - a, jod, grad)
                train._loss(jod, grad, target_dev[a:b], b - a, step_loss[i:i + 1], dloss)
                torch.mul(dloss, mask, out=theta.grad)
                opt.step()
                done += 1
                if steps is not None and done >= steps:
                    break
            got = step_loss[:i + 1].cpu().numpy()                     # one copy per epoch
            for k, v in enumerate(got):
                log.loss(epoch, epoch * len(cuts) + k, v)
            losses += [float(v) for v in got]
            if steps is not None and done >= steps:
                break
            if epoch % val_epoch == 0:
                validate(epoch)
    finally:
        log.close()
    latest = theta.detach().cpu().numpy().copy()
    if keeper.monitor is None or keeper.state is None:
        chosen, chosen_epoch = latest, epoch
    else:
        chosen, chosen_epoch = keeper.state, keeper.epoch
    return {"theta": chosen, "epoch": chosen_epoch, "theta_latest": latest, "losses": losses, "validation": validation}


def assign_theta(metric, theta, names):
    """The fitted entries of theta into the metric, through the path every parameter assignment takes (all or nothing)."""
    p = dict(metric.parameters)
    for n in names:
        a, b = THETA_SLOTS[n]
        v = [float(x) for x in theta[a:b]]
        p[n] = v if isinstance(p[n], list) else v[0]
    metric._set_parameters(p)


# ---------------------------------------------------------------- rescoring mode
def _band_values(parameters):
    v = np.zeros(BAND_COUNT, dtype=np.float64)
    for n, (a, b) in BAND_PARAMETERS.items():
        v[a:b] = np.asarray(parameters[n], dtype=np.float32).reshape(-1)
    return v


def _set_display(metric, display, config_paths):
    from .display_model import vvdp_display_geometry, vvdp_display_photometry
    photo = vvdp_display_photometry.load(display, config_paths=config_paths)
    geom = vvdp_display_geometry.load(display, config_paths=config_paths)
    metric.set_display_model(display_photometry=photo, display_geometry=geom)
    return photo, geom


def _source(row, args, photo, geom):
    from .video_source_file import video_source_file
    return video_source_file(os.path.join(args.path_prefix, row["test"]), os.path.join(args.path_prefix, row["reference"]),
                             display_photometry=photo, full_screen_resize=getattr(args, "full_screen_resize", None),
                             resize_resolution=geom.resolution, fps=getattr(args, "fps", None), verbose=getattr(args, "verbose", False),
                             config_paths=args.config_paths)


def _row_display(row, args):
    display = row.get("display") if args.display == "per-row" else args.display
    if not display:
        raise vq_exception('Please select a display name (-d), or include a column titled "display" and pass "--display per-row".')
    return display


def rescoring_step(metric, rows, args, theta, band, opt, masks, fitted):
    """One optimiser step of rescoring mode on the rows of a mini-batch: the metric gets the current values of the fitted parameters
    (fitted = (pooling names, band names)), every row is scored with
    predict_video_source_with_parameter_gradient() under its own display (band gradients, and the Q_per_ch it scored), the pooling
    gradients and the JOD come from cvvdp_pool_dataset on that Q_per_ch, and both are combined with 2 (jod - target) / n.
    Returns (loss, clips scored)."""
    dev = metric.device
    p = dict(metric.parameters)
    th, bd = theta.detach().cpu().numpy(), band.detach().cpu().numpy()
    for names, slots, values in ((fitted[0], THETA_SLOTS, th), (fitted[1], BAND_PARAMETERS, bd)):
        for n in names:                                                # as an assignment `metric.<name> = tensor` stores it: float32 values
            a, b = slots[n]
            p[n] = metric._parameter_value(n, values[a:b] if isinstance(p[n], list) else values[a], p[n])
    metric._set_parameters(p)
    qs, bands, targets = [], [], []
    for row in rows:
        photo, geom = _set_display(metric, _row_display(row, args), args.config_paths)
        _, grads = metric.predict_video_source_with_parameter_gradient(_source(row, args, photo, geom))
        Q = metric._param_grad_Q
        B = int(Q.shape[0])
        qs.append(Q)
        bands.append(torch.cat([grads[n].reshape(B, -1).double() for n in BAND_PARAMETERS], dim=1))
        targets += [float(row["jod"])] * B
    fs = FeatureSet.from_stats(qs, targets, device=dev)
    jod, grad = fs._pool(theta.detach(), _betas(betas_of(metric.parameters)), None, len(fs))
    target = fs.on_device()["target"]
    loss, dloss = fs._loss(jod, grad, target, len(fs))
    w = (2.0 / len(fs)) * (jod - target)
    torch.mul(dloss, masks[0], out=theta.grad)
    rows_band, acc = torch.cat(bands, dim=0), torch.zeros((BAND_COUNT,), dtype=torch.float64, device=dev)
    for k in range(len(fs)):                                           # the clips in order: a fixed summation order
        acc += w[k] * rows_band[k]
    torch.mul(acc, masks[1], out=band.grad)
    opt.step()
    return loss, len(fs)


def fit_rescoring(metric, train_rows, args, names, steps=None):
    """The full fit: Adam over the pooling parameters and the band parameters named in `names`, the clips scored again on every step.
    The metric ends with the fitted parameters; a refused or failed run leaves it with the ones it had.  Returns a dict: losses,
    clips_per_second, epoch."""
    pool_names, band_names = parameter_names(names)
    if not train_rows:
        raise vq_exception("fit: the training split is empty")
    for r in train_rows:
        if "jod" not in r:
            raise vq_exception("the table has no column 'jod'")
    before = dict(metric.parameters)
    before_display = (metric.display_photometry, metric.display_geometry)
    dev = metric.device
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device available: colorvideovdp_amd has no CPU path")
    theta = torch.from_numpy(theta_of(before)).to(dev).requires_grad_(True)
    band = torch.from_numpy(_band_values(before)).to(dev).requires_grad_(True)
    theta.grad, band.grad = torch.zeros_like(theta), torch.zeros_like(band)
    masks = (torch.from_numpy(_mask(pool_names, THETA_SLOTS, THETA_COUNT)).to(dev), torch.from_numpy(_mask(band_names, BAND_PARAMETERS, BAND_COUNT)).to(dev))
    opt = torch.optim.Adam([theta, band], lr=args.learning_rate)
    log = _Log(getattr(args, "log_dir", None))
    losses, clips, done, epoch = [], 0, 0, -1
    t0 = time.perf_counter()
    try:
        for epoch in range(args.num_epochs):
            perm, cuts = _batches(len(train_rows), args.batch, args.seed, epoch)
            for a, b in cuts:
                loss, n = rescoring_step(metric, [train_rows[k] for k in perm[a:b]], args, theta, band, opt, masks, (pool_names, band_names))
                losses.append(float(loss.cpu()))
                log.loss(epoch, done, losses[-1])
                clips += n
                done += 1
                if steps is not None and done >= steps:
                    break
            if steps is not None and done >= steps:
                break
        # the last step's values into the metric
        p = dict(metric.parameters)
        th, bd = theta.detach().cpu().numpy(), band.detach().cpu().numpy()
        for names_, slots, values in ((pool_names, THETA_SLOTS, th), (band_names, BAND_PARAMETERS, bd)):
            for n in names_:
                a, b = slots[n]
                p[n] = metric._parameter_value(n, values[a:b] if isinstance(p[n], list) else values[a], p[n])
        metric._set_parameters(p)
    except BaseException:
        metric._set_parameters(before)
        raise
    finally:
        log.close()
        metric.set_display_model(display_photometry=before_display[0], display_geometry=before_display[1])
    seconds = time.perf_counter() - t0
    return {"losses": losses, "clips_per_second": clips / seconds if seconds > 0 else float("nan"), "epoch": epoch,
            "theta": theta.detach().cpu().numpy(), "band": band.detach().cpu().numpy()}


# ---------------------------------------------------------------- the ML head (-m cvvdp-ml-saliency)
ML_MODEL = "cvvdp_ml_saliency"


def _ml_metric(args, random_init):
    from .cvvdp_ml_metric import cvvdp_ml_saliency
    display = args.display if args.display not in (None, "per-row") else "standard_4k"
    return cvvdp_ml_saliency(quiet=True, display_name=display, temp_padding="replicate", config_paths=args.config_paths, random_init=random_init)


def write_ml_features(fname, features, frames_per_second):
    """`band<k>` [F, H', W', C, 6] float32 of one clip (features: the list extract_features returns, batch 1), and its frame rate."""
    arrays = {}
    for k, f in enumerate(features):
        f = f.detach().cpu().numpy() if torch.is_tensor(f) else np.asarray(f)
        if f.ndim != 6 or f.shape[0] != 1 or f.shape[5] != 6:
            raise vq_exception(f"features of band {k} have shape {f.shape}, expected [1, F, H', W', C, 6]")
        arrays[f"band{k}"] = np.ascontiguousarray(f[0], dtype=np.float32)
    np.savez(fname, bands=np.int32(len(arrays)), frames_per_second=np.float64(frames_per_second), **arrays)


def read_ml_features(fname, device=None):
    """The list of [1, F, H', W', C, 6] float32 tensors write_ml_features stored."""
    if not os.path.isfile(fname):
        raise vq_exception(f'Features missing: "{fname}" (run `extract -m cvvdp-ml-saliency` first)')
    with np.load(fname, allow_pickle=False) as g:
        feats = [torch.from_numpy(g[f"band{k}"][None]) for k in range(int(g["bands"]))]
    return [f.to(device) for f in feats] if device is not None else feats


def write_ml_model(metric, output_dir, weights, baseband_weight, comment=None):
    """OUTPUT_DIR/cvvdp_ml_saliency/cvvdp.ckpt ({"state_dict": the networks of the packed `weights`}) and cvvdp_parameters.json (the
    metric's own parameter file with `baseband_weight` replaced), the layout cvvdp_ml_saliency(config_paths=[OUTPUT_DIR]) loads.
    Returns the directory."""
    from .config import json2dict
    from .cvvdp_ml_metric import unpack_weights
    out = os.path.join(output_dir, ML_MODEL)
    os.makedirs(out, exist_ok=True)
    torch.save({"state_dict": unpack_weights(weights, state_dict=True)}, os.path.join(out, "cvvdp.ckpt"))
    p = dict(json2dict(metric.parameters_file))
    p["baseband_weight"] = float(np.float32(baseband_weight))
    if comment:
        p["__comment"] = comment
    with open(os.path.join(out, "cvvdp_parameters.json"), "w") as f:
        json.dump(p, f, indent=4)
        f.write("\n")
    return out


def fit_ml(metric, train, val, fit_baseband=False, batch=4, learning_rate=1e-3, num_epochs=50, val_epoch=1, save="latest", seed=0,
           log_dir=None):
    """Adam on the mean squared error of the JOD over the packed weights of the metric's networks (and its baseband_weight), on stored
    features.  train, val: (list of feature lists, targets); val may be None.  Every clip of a mini-batch is one
    differentiable_jods() (forward head, and the HIP weight gradient in backward()).  Returns a dict: weights (float32 [ML_WEIGHTS],
    per --save), baseband_weight, epoch, losses (one per step), validation, jod_train (of the returned model)."""
    if batch < 1 or num_epochs < 0 or val_epoch < 1:
        raise vq_exception("fit: batch and val-epoch must be at least 1, num-epochs at least 0")
    keeper = _Keeper(save)
    dev = metric.device
    feats, targets = train
    if not feats:
        raise vq_exception("fit: the training split is empty")
    target = torch.as_tensor(np.asarray(targets, dtype=np.float32)).to(dev)
    w = metric.weight_tensor().requires_grad_(True)
    bw = torch.tensor(float(metric._ml_baseband_weight), dtype=torch.float32, device=dev, requires_grad=fit_baseband)
    opt = torch.optim.Adam([w, bw] if fit_baseband else [w], lr=learning_rate)
    log = _Log(log_dir)
    losses, validation = [], []

    def jods(clips):
        with torch.no_grad():
            return torch.cat([metric._head_forward(c, metric._weights_arg(w), float(bw)).reshape(-1)[:1] for c in clips])

    def state():
        return w.detach().clone(), float(bw.detach())

    def validate(epoch):
        if val is None:
            return
        score = measures(jods(val[0]).cpu().numpy(), val[1])
        validation.append((epoch, score))
        log.validation(epoch, score)
        logging.info(f"epoch {epoch}: validation rmse {score['rmse']:.4f} pearson {score['pearson']:.4f} spearman {score['spearman']:.4f}")
        keeper.offer(epoch, score, state)

    try:
        validate(-1)
        done, epoch = 0, -1
        for epoch in range(num_epochs):
            perm, cuts = _batches(len(feats), batch, seed, epoch)
            for a, b in cuts:
                opt.zero_grad(set_to_none=True)
                q = torch.cat([metric.differentiable_jods(feats[k], w, bw if fit_baseband else None).reshape(-1)[:1] for k in perm[a:b]])
                loss = ((q - target[torch.from_numpy(perm[a:b].astype(np.int64)).to(dev)]) ** 2).mean()
                loss.backward()
                opt.step()
                losses.append(float(loss.detach().cpu()))
                log.loss(epoch, done, losses[-1])
                done += 1
            if epoch % val_epoch == 0:
                validate(epoch)
    finally:
        log.close()
    if keeper.monitor is None or keeper.state is None:
        (weights, bw_out), chosen_epoch = state(), epoch
    else:
        (weights, bw_out), chosen_epoch = keeper.state, keeper.epoch
    with torch.no_grad():
        jod_train = torch.cat([metric._head_forward(c, metric._weights_arg(weights), bw_out).reshape(-1)[:1] for c in feats]).cpu().numpy()
    return {"weights": weights, "baseband_weight": bw_out, "epoch": chosen_epoch, "losses": losses, "validation": validation,
            "jod_train": jod_train}


def run_fit_ml(args, columns, rows, metric=None):
    """`fit -m cvvdp-ml-saliency`.  Returns (the result of fit_ml, the directory written)."""
    names = list(args.parameters or [])
    for n in names:
        if n != "baseband_weight":
            raise vq_exception(f"unknown parameter '{n}': with -m cvvdp-ml-saliency the networks are always fitted and --parameters may add baseband_weight")
    if args.split_column not in columns:
        raise vq_exception(f'Split column "{args.split_column}" not found')
    if "jod" not in columns:
        raise vq_exception("the table has no column 'jod'")
    if args.batch < 1:
        raise vq_exception("--batch must be at least 1")
    _Keeper(args.save)
    train_rows, test_rows = split_rows(rows, args.split_column, args.seed, args.train_ratio)
    if not train_rows:
        raise vq_exception("fit: the training split is empty")
    if metric is None:
        if args.ckpt is not None and not os.path.isfile(args.ckpt):
            raise vq_exception(f"--ckpt {args.ckpt}: no such file")
        with torch.random.fork_rng(devices=[]):                          # a seeded start that leaves the caller's generator alone
            torch.manual_seed(args.seed)
            metric = _ml_metric(args, random_init=True)
        if args.ckpt is not None:
            metric.load_state_dict_nets(torch.load(args.ckpt, map_location="cpu")["state_dict"])
    if not torch.cuda.is_available():
        raise RuntimeError("no HIP device available: colorvideovdp_amd has no CPU path")
    ft_path = features_dir(args.features_suffix)

    def load(rows_, split):
        if not rows_:
            return None
        return ([read_ml_features(os.path.join(ft_path, split, row_id(r["test"]) + "_mlfeat.npz"), metric.device) for r in rows_],
                [float(r["jod"]) for r in rows_])

    result = fit_ml(metric, load(train_rows, "train"), load(test_rows, "test"), fit_baseband="baseband_weight" in names, batch=args.batch,
                    learning_rate=args.learning_rate, num_epochs=args.num_epochs, val_epoch=args.val_epoch, save=args.save, seed=args.seed,
                    log_dir=args.log_dir)
    comment = (f"ColorVideoVDP-ML-Saliency parameters generated by the calibration tool. The networks in cvvdp.ckpt are fit on data from file "
               f"{args.quality_file} (epoch {result['epoch']}).")
    out = write_ml_model(metric, args.output_dir, result["weights"], result["baseband_weight"], comment)
    logging.info(f'New ColorVideoVDP-ML-Saliency checkpoint and parameters saved in "{out}"')
    return result, out


# ---------------------------------------------------------------- command line
def _common(p):
    p.add_argument("quality_file", help="Path to the .csv file with the quality scores.")
    p.add_argument("-s", "--split-column", default="reference", help="Column the train / test split is made on.")
    p.add_argument("-r", "--train-ratio", type=int, choices=range(100), default=80, metavar="0..99", help="Percentage of the conditions used for training.")
    p.add_argument("--seed", type=int, default=0, help="Random seed of the split (and of the mini-batch order).")
    p.add_argument("--masking", default="base", help="Only 'base' exists.")
    p.add_argument("--pooling", default="base", help="Only 'base' exists.")
    p.add_argument("-f", "--features-suffix", default=None, help="Suffix of the features directory.")
    p.add_argument("-c", "--config-paths", type=str, nargs="+", default=[], help="Paths to configuration files or directories.")
    p.add_argument("-p", "--path-prefix", default="", help="Prefix for each test and reference file.")
    p.add_argument("-d", "--display", default=None, help="Display name, or 'per-row' to take it from the column 'display'.")
    p.add_argument("--full-screen-resize", choices=["bilinear", "bicubic", "nearest", "area"], default=None)
    p.add_argument("--fps", type=float, default=None, help="Frames per second of .npy clips (files that carry a rate ignore it).")
    p.add_argument("-v", "--verbose", action="store_true", default=False)
    p.add_argument("-m", "--metric", choices=["cvvdp", "cvvdp-ml-saliency"], default="cvvdp",
                   help="The model to calibrate: the base model's parameters, or the networks of the ML head (needs -c with its parameter file).")


def make_parser():
    parser = argparse.ArgumentParser(prog="python -m colorvideovdp_amd.calibration", description="Calibrate ColorVideoVDP parameters for a new dataset")
    sub = parser.add_subparsers(dest="command", required=True)
    ex = sub.add_parser("extract", help="Score every row once and write its features.")
    _common(ex)
    ex.add_argument("-w", "--worker", default=None, type=str, help="k/N: this is worker k of N (k = 1..N).")
    ex.add_argument("--resume", action="store_true", default=False, help="Skip the rows whose feature file exists.")
    ft = sub.add_parser("fit", help="Fit parameters to the extracted features (or, with band parameters, by rescoring).")
    _common(ft)
    ft.add_argument("-o", "--output-dir", default="new_config", help="Directory the updated parameters are stored in.")
    ft.add_argument("-b", "--batch", type=int, default=4, help="Mini-batch size.")
    ft.add_argument("-lr", "--learning-rate", type=float, default=1e-3)
    ft.add_argument("-e", "--num-epochs", type=int, default=50)
    ft.add_argument("-l", "--log-dir", default="logs", help="Directory of log.csv (loss per step, measures per validation).")
    ft.add_argument("--val-epoch", type=int, default=1, help="Epochs between validations.")
    ft.add_argument("--save", choices=["latest", "best-rmse", "best-pearson", "best-spearman"], default="latest")
    ft.add_argument("--parameters", nargs="+", default=None,
                    help=f"Parameters to fit (default: {' '.join(DEFAULT_PARAMETERS)}; image_int may be added; any of {' '.join(BAND_PARAMETERS)} selects rescoring mode).")
    ft.add_argument("--resample-bands", action="store_true", default=False, help="Refused.")
    ft.add_argument("--ckpt", default=None, help="-m cvvdp-ml-saliency: the checkpoint to start from (default: a random initialisation seeded with --seed).")
    return parser


def parse_arguments(argv):
    """The command line, then the quality file's header behind it (the header overrides)."""
    parser = make_parser()
    args = parser.parse_args(argv)
    header, columns, rows = read_quality_file(args.quality_file)
    words = header_arguments(header, vars(args).keys())
    if words:
        args = parser.parse_args(list(argv) + words)
    if args.masking != "base" or args.pooling != "base":
        raise vq_exception(f"--masking {args.masking} --pooling {args.pooling}: only the base model exists (the mlp / lstm / gru variants are not part of this package)")
    if getattr(args, "resample_bands", False):
        raise vq_exception("--resample-bands is refused: the reference's resampling interpolates one channel only")
    return args, columns, rows


def run_extract(args, columns, rows, metric=None):
    """extract_features.py:79-151.  Returns the files written."""
    from .cvvdp_metric import cvvdp
    ml = getattr(args, "metric", "cvvdp") == "cvvdp-ml-saliency"
    if args.display is None:
        raise vq_exception('Please select a display name (-d), or include a column titled "display" and pass "--display per-row".')
    if args.display == "per-row" and "display" not in columns:
        raise vq_exception('Per-row display selected but cannot find column "display".')
    if args.split_column not in columns:
        raise vq_exception(f'Split column "{args.split_column}" not found')
    start, step = 0, 1
    if args.worker is not None:
        m = re.fullmatch(r"(\d+)/(\d+)", args.worker)
        if not m or not 1 <= int(m.group(1)) <= int(m.group(2)):
            raise vq_exception(f"--worker {args.worker}: expected k/N with 1 <= k <= N")
        start, step = int(m.group(1)) - 1, int(m.group(2))
        logging.info(f"Worker {start + 1} out of {step} workers.")
    train_cond = set(split_conditions([r[args.split_column] for r in rows], args.seed, args.train_ratio)[0])
    ft_path = features_dir(args.features_suffix)
    if metric is None and ml:
        with torch.random.fork_rng(devices=[]):                      # (the features do not depend on the networks, and the caller's
            metric = _ml_metric(args, random_init=True)              # generator is not the one to draw them from)
    if metric is None:
        metric = cvvdp(quiet=True, display_name="standard_4k" if args.display == "per-row" else args.display, temp_padding="replicate",
                       config_paths=args.config_paths)
    for split in ("train", "test"):
        os.makedirs(os.path.join(ft_path, split), exist_ok=True)
    written = []
    for kk in range(start, len(rows), step):
        row = rows[kk]
        rid = row_id(row["test"])
        dest = os.path.join(ft_path, "train" if row[args.split_column] in train_cond else "test", rid + ("_mlfeat.npz" if ml else "_fmap.json"))
        if args.resume and os.path.isfile(dest):
            logging.info(f"Skipping condition {rid}")
            continue
        photo, geom = _set_display(metric, _row_display(row, args), args.config_paths)
        try:
            with torch.no_grad():
                if ml:
                    vs, _, feats = metric._source_features(_source(row, args, photo, geom))
                else:
                    _, stats = metric.predict_video_source(_source(row, args, photo, geom))
        except Exception:
            logging.error(f"Failed on condition {rid}")
            raise
        if ml:
            write_ml_features(dest, feats, vs.get_frames_per_second())
        else:
            metric.write_features_to_json(stats, dest)
        written.append(dest)
    return written


def _feature_set(rows, split, args, device):
    if not rows:
        return None
    for r in rows:
        if "jod" not in r:
            raise vq_exception("the table has no column 'jod'")
    ft_path = features_dir(args.features_suffix)
    ids = [row_id(r["test"]) for r in rows]
    return FeatureSet.from_files([os.path.join(ft_path, split, i + "_fmap.json") for i in ids], [float(r["jod"]) for r in rows], device=device, ids=ids)


def run_fit(args, columns, rows, metric=None):
    """train.py:60-169.  Returns (the result of the fit, the parameter file written)."""
    from .cvvdp_metric import cvvdp
    if getattr(args, "metric", "cvvdp") == "cvvdp-ml-saliency":
        return run_fit_ml(args, columns, rows, metric)
    pool_names, band_names = parameter_names(args.parameters)
    if args.split_column not in columns:
        raise vq_exception(f'Split column "{args.split_column}" not found')
    if "jod" not in columns:
        raise vq_exception("the table has no column 'jod'")
    if args.batch < 1:
        raise vq_exception("--batch must be at least 1")
    _Keeper(args.save)
    train_rows, test_rows = split_rows(rows, args.split_column, args.seed, args.train_ratio)
    if not train_rows:
        raise vq_exception("fit: the training split is empty")
    if metric is None:
        display = args.display if args.display not in (None, "per-row") else "standard_4k"
        metric = cvvdp(quiet=True, display_name=display, temp_padding="replicate", config_paths=args.config_paths)
    if band_names:
        result = fit_rescoring(metric, train_rows, args, pool_names + band_names)
        logging.info(f"rescoring mode: {result['clips_per_second']:.2f} clips per second")
        print(f"rescoring mode: {result['clips_per_second']:.2f} clips per second", file=sys.stderr)
    else:
        train = _feature_set(train_rows, "train", args, metric.device)
        val = _feature_set(test_rows, "test", args, metric.device)
        result = fit_features(train, val, metric.parameters, pool_names, batch=args.batch, learning_rate=args.learning_rate,
                              num_epochs=args.num_epochs, val_epoch=args.val_epoch, save=args.save, seed=args.seed, log_dir=args.log_dir)
        assign_theta(metric, result["theta"], pool_names)
    os.makedirs(args.output_dir, exist_ok=True)
    out = os.path.join(args.output_dir, "cvvdp_parameters.json")
    comment = (f"ColourVideoVDP parameters generated by calibration tool (calibration/train.py). Some parameters are fit on data from file "
               f"{args.quality_file} (epoch {result['epoch']}).")
    metric.save_to_config(out, comment)
    logging.info(f'New ColorVideoVDP parameters saved in "{out}"')
    return result, out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    try:
        args, columns, rows = parse_arguments(argv)
        logging.basicConfig(format="[%(levelname)s] %(message)s", level=logging.DEBUG if args.verbose else logging.INFO)
        if args.command == "extract":
            run_extract(args, columns, rows)
        else:
            run_fit(args, columns, rows)
    except vq_exception as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
