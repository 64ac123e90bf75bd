"""Fitting a classifier head on frozen scene embeddings, on the GPU (acx_head_fit_step in include/acx.h).

The reference fine-tunes with the whole model in train mode (pytorch/finetune_audiocaps.py: base frozen, BCELoss on
clipwise_output, optim.Adam(lr=1e-4, amsgrad=True), mAP per epoch).  With the backbone frozen the head's input -- the scene
embedding -- never changes, so the embeddings are computed once and the training is logits = E W^T + b, binary cross-entropy,
Adam / AdamW, two launches per step:

    from audioset_convnext_inf_amd.pytorch.finetune import fit_head
    fit = fit_head(emb, target, epochs=20, batch_size=64, lr=1e-4)     # emb (n, 768) fp32 CUDA, target (n, N) bool / uint8 / float
    fit.weight, fit.bias, fit.loss                                     # (N, 768), (N,), (steps,) on the device
    fit.history                                                        # per epoch: mean loss and, with val=, mAP / AUC / d'

A single-label head (one class per clip: ESC-50, "one folder per class") is trained with softmax cross-entropy instead:

    fit = fit_head(emb, labels, classes=50, loss="ce", label_smoothing=0.1)        # labels (n,) integers, or (n, N) one-hot rows

(acx_head_fit_step_ce: three launches per step), read with pytorch/classify.py softmax_topk and judged with
classification_metrics.  loss="bce" (the default) is the path above, bit for bit.

Many fits over the same embeddings -- the folds of a cross-validation, the settings of a grid -- advance together, each stage one
launch for all of them (acx_head_fit_group_step), every head bit-equal to its fit_head call:

    fits = fit_heads(emb, target, [dict(rows=train_rows, val=held_rows, lr=1e-3), ...], epochs=20)
    cv = cross_validate_head(emb, labels, folds=5, grid={"lr": [1e-4, 1e-3]}, loss="ce", classes=50)   # cv.scores, cv.best, cv.final

The epoch order is part of the contract: torch.randperm(n, generator=g) drawn once per epoch from ONE CPU generator
g = torch.Generator().manual_seed(seed) (shuffle=False: arange); the last batch of an epoch is short unless drop_last.  The
initial weights (init=None) come from a second generator seeded with `seed` too: trunc_normal_(std=0.02) weight, zero bias
(convnext.py:263-267).  Every step of a fit is enqueued on the current stream without a host synchronisation."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from .. import _ffi
from .._ffi import vp
from . import _inputs

EMBED_DIM = 768
HeadFit = namedtuple("HeadFit", ["weight", "bias", "loss", "history"])


def epoch_batches(n, batch_size, drop_last=False):
    """[(start, rows)] of the mini-batches of one epoch over a permutation of n rows: consecutive runs of batch_size, the last
    one short unless drop_last."""
    n, batch_size = int(n), int(batch_size)
    full = n // batch_size
    out = [(i * batch_size, batch_size) for i in range(full)]
    if n % batch_size and not drop_last:
        out.append((full * batch_size, n % batch_size))
    return out


def epoch_orders(n, epochs, seed=0, shuffle=True):
    """(epochs, n) int64 CPU tensor: row e is the order in which epoch e visits the data set (see the module docstring)."""
    g = torch.Generator().manual_seed(int(seed))
    rows = [torch.randperm(n, generator=g) if shuffle else torch.arange(n) for _ in range(int(epochs))]
    return torch.stack(rows) if rows else torch.empty((0, n), dtype=torch.int64)


def init_head(classes, seed=0):
    """(weight (N, 768), bias (N,)) as the model initialises head_audioset (convnext.py:263-267): trunc_normal_(std=0.02) from a
    CPU generator seeded with `seed`, zero bias."""
    g = torch.Generator().manual_seed(int(seed))
    w = torch.empty(int(classes), EMBED_DIM)
    torch.nn.init.trunc_normal_(w, std=0.02, generator=g)
    return w, torch.zeros(int(classes))


def _check_hyper(epochs, batch_size, betas, eps, weight_decay):
    if isinstance(epochs, bool) or not isinstance(epochs, int) or epochs < 0:
        raise ValueError("epochs must be an integer >= 0 (got %r)" % (epochs,))
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError("batch_size must be an integer >= 1 (got %r)" % (batch_size,))
    if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
        raise ValueError("betas must be two values in [0, 1) (got %r)" % (betas,))
    if not float(eps) > 0.0:
        raise ValueError("eps must be > 0 (got %r)" % (eps,))
    if not float(weight_decay) >= 0.0:
        raise ValueError("weight_decay must be >= 0 (got %r)" % (weight_decay,))


def _lr_schedule(lr, steps):
    """One learning rate per step: a float repeated, or the caller's sequence (its length must be the step count)."""
    if isinstance(lr, (int, float)):
        lrs = [float(lr)] * steps
        bad = not (float(lr) >= 0.0 and np.isfinite(float(lr)))
    else:
        lrs = [float(v) for v in lr]
        if len(lrs) != steps:
            raise ValueError("lr has %d values for %d steps (one value per step, or one float)" % (len(lrs), steps))
        bad = any(not (v >= 0.0 and np.isfinite(v)) for v in lrs)
    if bad:
        raise ValueError("lr must be finite and >= 0")
    return lrs


def _check_pair(emb, target, name="emb", tname="target"):
    """Shapes, dtypes, devices and values of one (embeddings, targets) pair; -> (emb, target tensor for the kernel, dtype code)."""
    emb = _check_emb(emb, name)
    t = _check_target(target, int(emb.shape[0]), emb.device, name, tname)
    return emb, t, _inputs.target_code(t)


def _check_target(target, n, device, name="emb", tname="target"):
    """(n, N) multi-label targets on `device`, checked; -> the tensor the kernels read (uint8 or float32, rows in place)."""
    if not isinstance(target, torch.Tensor) or target.dim() != 2 or target.shape[0] != n:
        raise ValueError("%s must be a (%d, N) tensor (got %s)" % (tname, n, getattr(target, "shape", type(target))))
    if target.device != device:
        raise ValueError("%s is on %s, %s on %s" % (tname, target.device, name, device))
    N = int(target.shape[1])
    if not 1 <= N <= _ffi.MAX_CLASSES:
        raise ValueError("%s has N = %d classes (expected 1 .. %d)" % (tname, N, _ffi.MAX_CLASSES))
    if target.dtype == torch.bool:
        t = target.view(torch.uint8)
    elif target.dtype.is_floating_point:
        t = target if target.dtype == torch.float32 else target.to(torch.float32)
        if not bool(((t >= 0) & (t <= 1)).all()):
            raise ValueError("%s holds values outside [0, 1]" % tname)
    elif target.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        if not bool(((target == 0) | (target == 1)).all()):
            raise ValueError("%s holds values other than 0 and 1" % tname)
        t = target if target.dtype == torch.uint8 else target.to(torch.uint8)
    else:
        raise ValueError("%s must be bool, an integer type or floating point (got %s)" % (tname, target.dtype))
    return _inputs.rows(t)


def _check_emb(emb, name="emb", device=True):
    """Shape, dtype and (device=True) device of the embeddings; -> emb in a layout the kernels take (unit column stride, 16-byte
    aligned rows)."""
    if not isinstance(emb, torch.Tensor) or emb.dim() != 2 or emb.shape[1] != EMBED_DIM:
        raise ValueError("%s must be a (n, %d) tensor (got %s)" % (name, EMBED_DIM, getattr(emb, "shape", type(emb))))
    if emb.dtype != torch.float32:
        raise ValueError("%s must be float32 (got %s)" % (name, emb.dtype))
    if emb.shape[0] < 1:
        raise ValueError("%s holds no rows" % name)
    if not device:
        return emb
    if not emb.is_cuda:
        raise ValueError("%s must be a CUDA (HIP) tensor: fit_head runs on the GPU only (got device %s)" % (name, emb.device))
    return _inputs.rows(emb, align4=True)


def labels_of(target, n, classes=None, tname="target"):
    """The (n,) int64 labels and the class count N of a loss="ce" target: (n,) integer class numbers (classes= required, every
    label in [0, classes)), or (n, N) rows holding exactly one 1 and zeros otherwise.  Validates on the target's device (one
    synchronisation) and raises ValueError; -> (labels, N)."""
    if not isinstance(target, torch.Tensor):
        target = torch.as_tensor(np.asarray(target))
    if target.dim() == 1:
        if target.shape[0] != n:
            raise ValueError("%s must hold %d labels (got %s)" % (tname, n, tuple(target.shape)))
        if target.dtype == torch.bool or target.dtype.is_floating_point or target.dtype.is_complex:
            raise ValueError("%s of shape (n,) must be an integer tensor of class numbers (got %s)" % (tname, target.dtype))
        if classes is None:
            raise ValueError("classes= is required with (n,) integer labels")
        N = int(classes)
        if not 1 <= N <= _ffi.MAX_CLASSES:
            raise ValueError("classes = %d (expected 1 .. %d)" % (N, _ffi.MAX_CLASSES))
        lab = target.to(torch.int64)
        if n and not bool(((lab >= 0) & (lab < N)).all()):
            raise ValueError("%s holds labels outside [0, %d)" % (tname, N))
        return lab.contiguous(), N
    if target.dim() != 2 or target.shape[0] != n:
        raise ValueError("%s must be (%d,) labels or (%d, N) one-hot rows (got %s)" % (tname, n, n, tuple(target.shape)))
    N = int(target.shape[1])
    if not 1 <= N <= _ffi.MAX_CLASSES:
        raise ValueError("%s has N = %d classes (expected 1 .. %d)" % (tname, N, _ffi.MAX_CLASSES))
    if classes is not None and int(classes) != N:
        raise ValueError("classes = %d, but %s has %d columns" % (int(classes), tname, N))
    t = target.to(torch.float32)
    if not bool(((t == 0) | (t == 1)).all()):
        raise ValueError("%s holds values other than 0 and 1" % tname)
    if not bool((t.sum(dim=1) == 1).all()):
        raise ValueError("%s must hold exactly one 1 per row for loss=\"ce\" (a row with none or several was found)" % tname)
    return t.argmax(dim=1).to(torch.int64).contiguous(), N


def _validate_ce(weight, bias, emb_val, labels_val):
    from .classify import classification_metrics
    N = int(weight.shape[0])
    m = classification_metrics(labels_val, torch.addmm(bias, emb_val, weight.t()), k=min(5, N), confusion=False)
    return {"accuracy": m.accuracy, "topk_accuracy": m.topk_accuracy, "macro_f1": m.macro_f1}


def _validate(weight, bias, emb_val, target_val):
    from .metrics import tagging_metrics
    probs = torch.sigmoid(torch.addmm(bias, emb_val, weight.t()))
    stats = tagging_metrics(target_val, probs)
    return {"average_precision": stats["average_precision"], "auc": stats["auc"], "d_prime": stats["d_prime"],
            "mAP": float(np.mean(stats["average_precision"])), "mAUC": float(np.nanmean(stats["auc"]))}


def _check_val_ce(val, N, device):
    emb_val = _check_emb(val[0], "emb_val")
    return emb_val, labels_of(val[1], int(emb_val.shape[0]), N, "labels_val")[0].to(device)


def _check_val(val, N, device):
    emb_val, target_val, _ = _check_pair(val[0], val[1], "emb_val", "target_val")
    if target_val.shape[1] != N:
        raise ValueError("target_val has %d classes, target %d" % (target_val.shape[1], N))
    return emb_val, target_val


# What differs between the two losses of fit_head, picked once: the workspace query, the name of the step entry, its arguments
# between n_rows_total and idx (the kernel's target) and between rows and W, and how val= is checked and scored.
_Loss = namedtuple("_Loss", ["workspace_bytes", "step", "target_args", "class_args", "check_val", "validate"])


def _check_loss(loss, label_smoothing, classes):
    """The loss settings of fit_head / fit_heads; -> (ce, label_smoothing as a float)."""
    if loss not in ("bce", "ce"):
        raise ValueError("loss must be \"bce\" or \"ce\" (got %r)" % (loss,))
    label_smoothing = float(label_smoothing)
    ce = loss == "ce"
    if not ce and label_smoothing != 0.0:
        raise ValueError("label_smoothing belongs to loss=\"ce\"; binary cross-entropy takes soft targets instead")
    if not ce and classes is not None:
        raise ValueError("classes= belongs to loss=\"ce\"; with loss=\"bce\" the class count is the target's width")
    if ce and not 0.0 <= label_smoothing < 1.0:
        raise ValueError("label_smoothing must be in [0, 1) (got %r)" % (label_smoothing,))
    return ce, label_smoothing


def _check_data(emb, target, ce, label_smoothing, classes):
    """The (embeddings, targets) of a fit, checked; -> (emb, the kernel's target tensor, N, the loss's _Loss)."""
    if ce:
        _check_emb(emb, device=False)
        tgt, N = labels_of(target, int(emb.shape[0]), classes)     # the target's own errors come before the GPU-only one
        emb = _check_emb(emb)
        if isinstance(target, torch.Tensor) and target.device != emb.device:
            raise ValueError("target is on %s, emb on %s" % (target.device, emb.device))
        tgt = tgt.to(emb.device)
        how = _Loss(_ffi.head_fit_ce_workspace_bytes, "acx_head_fit_step_ce", (vp(tgt),), (N, label_smoothing), _check_val_ce,
                    _validate_ce)
    else:
        emb, tgt, tdtype = _check_pair(emb, target)
        N = int(tgt.shape[1])
        how = _Loss(_ffi.head_fit_workspace_bytes, "acx_head_fit_step", (vp(tgt), tdtype, tgt.stride(0)), (N,), _check_val, _validate)
    return emb, tgt, N, how


def _check_init(init, N):
    if len(init) != 2:
        raise ValueError("init must be (weight, bias)")
    w0, b0 = init
    if tuple(w0.shape) != (N, EMBED_DIM) or tuple(b0.shape) != (N,):
        raise ValueError("init must be a (%d, %d) weight and a (%d,) bias (got %s and %s)"
                         % (N, EMBED_DIM, N, tuple(w0.shape), tuple(b0.shape)))
    return w0, b0


def fit_head(emb, target, epochs=20, batch_size=64, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=True,
             decoupled=False, init=None, seed=0, shuffle=True, drop_last=False, val=None, loss="bce", label_smoothing=0.0,
             classes=None):
    """Train an nn.Linear(768, N) head on (n, 768) scene embeddings with binary cross-entropy and Adam (decoupled=True: AdamW);
    the defaults are the reference's fine-tuning settings.  lr: a float, or one value per step.  init: None (seeded
    trunc_normal(std=0.02) weight, zero bias) or (weight, bias) to continue from a head; the moments always start at zero.
    val: (emb_val, target_val) -> per-epoch tagging_metrics in the history (this synchronises once per epoch).
    loss="ce": softmax cross-entropy for a single-label head (F.cross_entropy with label_smoothing in [0, 1)); target is (n,)
    integer labels with classes=N, or (n, N) one-hot rows (labels_of); val=(emb_val, labels_val) puts accuracy, topk_accuracy
    (k = min(5, N)) and macro_f1 into the history.
    Returns HeadFit(weight, bias, loss, history): device tensors and a list of one dict per epoch, whose "loss" is a 0-d
    device tensor (the mean of the epoch's step losses)."""
    ce, label_smoothing = _check_loss(loss, label_smoothing, classes)
    _check_hyper(epochs, batch_size, betas, eps, weight_decay)
    emb, tgt, N, how = _check_data(emb, target, ce, label_smoothing, classes)
    n, device = int(emb.shape[0]), emb.device
    if val is not None:
        if len(val) != 2:
            raise ValueError("val must be (emb_val, target_val)")
        emb_val, target_val = how.check_val(val, N, device)
        if emb_val.device != device:
            raise ValueError("emb_val is on %s, emb on %s" % (emb_val.device, device))
    if init is None:
        w0, b0 = init_head(N, seed)
    else:
        w0, b0 = _check_init(init, N)
    batches = epoch_batches(n, batch_size, drop_last)
    steps = epochs * len(batches)
    lrs = _lr_schedule(lr, steps)

    with torch.no_grad(), torch.cuda.device(device):
        W = w0.detach().to(device=device, dtype=torch.float32, copy=True).contiguous()
        b = b0.detach().to(device=device, dtype=torch.float32, copy=True).contiguous()
        loss = torch.zeros(steps, dtype=torch.float32, device=device)
        history = []
        if steps == 0:
            return HeadFit(W, b, loss, history)
        order = epoch_orders(n, epochs, seed, shuffle).to(device)
        mom = torch.zeros((3, N, EMBED_DIM), dtype=torch.float32, device=device)
        momb = torch.zeros((3, N), dtype=torch.float32, device=device)
        status = torch.zeros(1, dtype=torch.int32, device=device)
        ws_bytes = how.workspace_bytes(min(batch_size, n), N)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        step_fn = getattr(_ffi.lib(), how.step)
        hp = _ffi.adam(betas[0], betas[1], eps, weight_decay, amsgrad, decoupled)
        stream = _ffi.stream_ptr(device)
        fixed_a = (vp(emb), emb.stride(0), n) + how.target_args
        fixed_b = how.class_args + (
            vp(W), vp(b), vp(mom[0]), vp(mom[1]), vp(mom[2]) if amsgrad else None, vp(momb[0]), vp(momb[1]),
            vp(momb[2]) if amsgrad else None, ctypes.byref(hp))
        tail = (vp(status), vp(ws), ws_bytes, stream)
        order_ptr, loss_ptr = order.data_ptr(), loss.data_ptr()
        t = 0
        for e in range(epochs):
            for start, rows in batches:
                rc = step_fn(*fixed_a, ctypes.c_void_p(order_ptr + 8 * (e * n + start)), rows, *fixed_b, t + 1, lrs[t],
                             ctypes.c_void_p(loss_ptr + 4 * t), *tail)
                if rc != _ffi.OK:
                    _ffi.check(rc)
                t += 1
            rec = {"epoch": e, "loss": loss[e * len(batches):(e + 1) * len(batches)].mean()}
            if val is not None:
                rec.update(how.validate(W, b, emb_val, target_val))
            history.append(rec)
    return HeadFit(W, b, loss, history)


# ---- many heads at once: groups of fits, k-fold cross-validation, grids ---------------------------------------------------------
# A small fit is bound by launch latency: a step of (n 2 000, N 50, batch 64) occupies 16 + 192 workgroups of a 256-CU part.
# fit_heads advances up to FIT_MAX_JOBS independent fits over the SAME embeddings per launch (acx_head_fit_group_step); every
# head has the bits of the fit_head call it replaces.

_JOB_DEFAULTS = {"rows": None, "lr": 1e-4, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.0, "seed": 0, "init": None,
                 "val": None}
GRID_JOB_KEYS = ("lr", "weight_decay", "betas", "eps", "seed")                   # what the jobs of one group may differ in
GRID_SHARED_KEYS = ("epochs", "batch_size", "label_smoothing", "amsgrad", "decoupled", "shuffle", "drop_last")
CrossValidation = namedtuple("CrossValidation", ["configs", "fold_ids", "metric", "scores", "mean", "std", "best", "fits", "final"])


def group_schedule(sizes, epochs, batch_size, drop_last=False):
    """(steps, J) int32 numpy array: the rows job j (a training set of sizes[j] rows) has in each step of a group fit.  An epoch
    of the group takes as many steps as its longest job's epoch; job j runs its own epoch_batches(sizes[j], ...) in the first
    steps of each epoch and sits the rest out (0 rows)."""
    per = [epoch_batches(m, batch_size, drop_last) for m in sizes]
    spe = max([len(b) for b in per], default=0)
    rows = np.zeros((int(epochs) * spe, len(per)), dtype=np.int32)
    for j, b in enumerate(per):
        for k, (_, r) in enumerate(b):
            rows[k::spe, j] = r
    return rows


def _check_index(rows, n, name, device):
    """A (m,) int64 tensor of row numbers in [0, n), on the CPU or on `device`; -> its CPU copy."""
    if not isinstance(rows, torch.Tensor) or rows.dim() != 1 or rows.dtype != torch.int64:
        raise ValueError("%s must be a (m,) int64 tensor of row numbers (got %s)"
                         % (name, getattr(rows, "dtype", type(rows))))
    if rows.shape[0] < 1:
        raise ValueError("%s holds no rows" % name)
    if rows.device.type != "cpu" and rows.device != device:
        raise ValueError("%s is on %s, emb on %s" % (name, rows.device, device))
    r = rows.cpu()
    if int(r.min()) < 0 or int(r.max()) >= n:
        raise ValueError("%s holds row numbers outside [0, %d)" % (name, n))
    return r


def _check_jobs(jobs, n, device, epochs, batch_size, drop_last):
    """The job list of fit_heads with the defaults filled in, rows / val as CPU tensors (None: all rows / no validation) and
    lr as the list of the job's steps."""
    if not isinstance(jobs, (list, tuple)) or len(jobs) == 0:
        raise ValueError("jobs must be a non-empty list of dicts")
    out = []
    for j, job in enumerate(jobs):
        if not isinstance(job, dict) or set(job) - set(_JOB_DEFAULTS):
            raise ValueError("jobs[%d] must be a dict with keys among %s (got %r)" % (j, sorted(_JOB_DEFAULTS), job))
        job = dict(_JOB_DEFAULTS, **job)
        _check_hyper(epochs, batch_size, job["betas"], job["eps"], job["weight_decay"])
        if job["rows"] is not None:
            job["rows"] = _check_index(job["rows"], n, "jobs[%d][\"rows\"]" % j, device)
        if job["val"] is not None:
            job["val"] = _check_index(job["val"], n, "jobs[%d][\"val\"]" % j, device)
        job["size"] = n if job["rows"] is None else int(job["rows"].shape[0])
        job["steps"] = epochs * len(epoch_batches(job["size"], batch_size, drop_last))
        job["lr"] = _lr_schedule(job["lr"], job["steps"])
        out.append(job)
    return out


def fit_heads(emb, target, jobs, epochs=20, batch_size=64, loss="bce", label_smoothing=0.0, classes=None, amsgrad=True,
              decoupled=False, shuffle=True, drop_last=False):
    """Train many heads over the same embeddings at once.  jobs: a list of dicts, each with any of
        rows=None | (m,) int64 row numbers of emb (the job's training set), lr (a float or one value per step OF THAT JOB), betas,
        eps, weight_decay, seed, init (fit_head's), val=None | (v,) int64 row numbers (held out: the metrics of fit_head's val=
        after the last epoch, in the last record of the history)
    -> [HeadFit] in job order.  fits[j].weight / .bias / .loss equal, bit for bit, fit_head(emb[rows], target[rows], ...) with
    the job's settings and the shared ones: job j visits rows[epoch_orders(len(rows), epochs, seed)[e]] in epoch e, gathered
    through the batch indices -- no copy of a subset is made for training.  Every step of a group advances all its jobs (each
    stage is one launch); jobs whose epoch has fewer batches sit the last steps of each epoch out (group_schedule).  More than
    FIT_MAX_JOBS jobs run as several groups.  Nothing synchronises per step or per epoch."""
    ce, label_smoothing = _check_loss(loss, label_smoothing, classes)
    _check_emb(emb, device=False)
    n = int(emb.shape[0])
    jobs = _check_jobs(jobs, n, emb.device, epochs, batch_size, drop_last)      # the jobs' own errors come before the GPU-only one
    emb, tgt, N, how = _check_data(emb, target, ce, label_smoothing, classes)
    inits = [init_head(N, job["seed"]) if job["init"] is None else _check_init(job["init"], N) for job in jobs]
    fits = []
    for lo in range(0, len(jobs), _ffi.FIT_MAX_JOBS):
        fits += _fit_group(emb, tgt, N, how, ce, label_smoothing, jobs[lo:lo + _ffi.FIT_MAX_JOBS], inits[lo:lo + _ffi.FIT_MAX_JOBS],
                           epochs, batch_size, amsgrad, decoupled, shuffle, drop_last)
    return fits


def _fit_group(emb, tgt, N, how, ce, label_smoothing, jobs, inits, epochs, batch_size, amsgrad, decoupled, shuffle, drop_last):
    n, device, J = int(emb.shape[0]), emb.device, len(jobs)
    sizes = [job["size"] for job in jobs]
    rows = group_schedule(sizes, epochs, batch_size, drop_last)
    steps = rows.shape[0]
    spe = steps // epochs if epochs else 0
    with torch.no_grad(), torch.cuda.device(device):
        W = torch.stack([w.detach().to(device=device, dtype=torch.float32) for w, _ in inits]).contiguous()
        b = torch.stack([v.detach().to(device=device, dtype=torch.float32) for _, v in inits]).contiguous()
        max_steps = max(job["steps"] for job in jobs)
        loss = torch.zeros((J, max_steps), dtype=torch.float32, device=device)
        if steps:
            # job j's batches of all epochs, one after the other: rows_j[order of epoch e]; the plan holds each step's offset
            orders, starts, at = [], [], 0
            for job in jobs:
                o = epoch_orders(job["size"], epochs, job["seed"], shuffle)
                orders.append((o if job["rows"] is None else job["rows"][o]).reshape(-1))
                starts.append(at)
                at += orders[-1].numel()
            idx = torch.cat(orders).to(device)
            idx_off = np.zeros((epochs, spe, J), dtype=np.int64)
            lrs = np.zeros((epochs, spe, J), dtype=np.float64)
            for j, job in enumerate(jobs):
                first = np.array([start for start, _ in epoch_batches(sizes[j], batch_size, drop_last)], dtype=np.int64)
                idx_off[:, :len(first), j] = np.arange(epochs, dtype=np.int64)[:, None] * sizes[j] + first[None, :]
                lrs[:, :len(first), j] = np.asarray(job["lr"], dtype=np.float64).reshape(epochs, len(first))
            idx_off, lrs = idx_off.reshape(steps, J), lrs.reshape(steps, J)
            hps = [_ffi.adam(job["betas"][0], job["betas"][1], job["eps"], job["weight_decay"], amsgrad, decoupled) for job in jobs]
            code = _ffi.FIT_LOSS_CE if ce else _ffi.FIT_LOSS_BCE
            rows_max = min(batch_size, max(sizes))
            plan = torch.from_numpy(_ffi.head_fit_plan(rows, idx_off, lrs, hps, rows_max, N, code)).to(device)
            mom = torch.zeros((J, 3, N, EMBED_DIM), dtype=torch.float32, device=device)
            momb = torch.zeros((J, 3, N), dtype=torch.float32, device=device)
            table = (_ffi.AcxFitJob * J)()
            for j in range(J):
                t = table[j]
                t.idx, t.W, t.b, t.loss = idx.data_ptr() + 8 * starts[j], W[j].data_ptr(), b[j].data_ptr(), loss[j].data_ptr()
                t.mW, t.vW, t.mb, t.vb = mom[j, 0].data_ptr(), mom[j, 1].data_ptr(), momb[j, 0].data_ptr(), momb[j, 1].data_ptr()
                t.vmaxW, t.vmaxb = (mom[j, 2].data_ptr(), momb[j, 2].data_ptr()) if amsgrad else (None, None)
            table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(device)
            status = torch.zeros(J, dtype=torch.int32, device=device)
            ws_bytes = _ffi.head_fit_group_workspace_bytes(J, rows_max, N, code)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
            step_fn = getattr(_ffi.lib(), "acx_head_fit_group_step_ce" if ce else "acx_head_fit_group_step")
            head = (vp(emb), emb.stride(0), n) + how.target_args + (J, rows_max) + how.class_args + (vp(table), vp(plan), steps)
            tail = (vp(status), vp(ws), ws_bytes, _ffi.stream_ptr(device))
            for s in range(steps):
                rc = step_fn(*head, s, *tail)
                if rc != _ffi.OK:
                    _ffi.check(rc)
        fits = []
        for j, job in enumerate(jobs):
            lj = loss[j, :job["steps"]]
            means = lj.view(epochs, -1).mean(dim=1) if job["steps"] else None
            history = [{"epoch": e, "loss": means[e]} for e in range(epochs)] if job["steps"] else []
            if job["val"] is not None and history:
                v = job["val"].to(device)
                history[-1].update(how.validate(W[j], b[j], emb[v], tgt[v]))
            fits.append(HeadFit(W[j], b[j], lj, history))
    return fits


def kfold_ids(n, folds, seed=0, labels=None):
    """(n,) int64 CPU tensor of fold numbers in [0, folds).  perm = torch.randperm(n, generator=Generator().manual_seed(seed));
    plain: row perm[i] goes to fold i % folds.  labels ((n,) integers): the rows of perm are first sorted stably by label and
    then dealt round-robin WITHOUT restarting at class boundaries, so every class's counts, and the fold sizes, differ by at
    most one between folds."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError("n must be an integer >= 1 (got %r)" % (n,))
    if isinstance(folds, bool) or not isinstance(folds, int) or not 2 <= folds <= n:
        raise ValueError("folds must be an integer in 2 .. n = %d (got %r)" % (n, folds))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed)))
    if labels is not None:
        if not isinstance(labels, torch.Tensor):
            labels = torch.as_tensor(np.asarray(labels))
        if labels.dim() != 1 or labels.shape[0] != n:
            raise ValueError("stratified folds need (n,) class numbers: multi-label targets cannot be stratified (got shape %s)"
                             % (tuple(labels.shape),))
        if labels.dtype == torch.bool or labels.dtype.is_floating_point or labels.dtype.is_complex:
            raise ValueError("labels must be an integer tensor of class numbers (got %s)" % labels.dtype)
        perm = perm[torch.sort(labels.cpu().to(torch.int64)[perm], stable=True).indices]
    ids = torch.empty(n, dtype=torch.int64)
    ids[perm] = torch.arange(n) % folds
    return ids


def expand_grid(grid):
    """The configs of a grid, as a list of dicts: None -> [{}]; a dict of lists -> their product in key order (the first key
    varies slowest); a list of dicts -> itself.  Keys: GRID_JOB_KEYS and GRID_SHARED_KEYS."""
    if grid is None:
        return [{}]
    if isinstance(grid, dict):
        if not grid:
            return [{}]
        keys = list(grid)
        for k in keys:
            if isinstance(grid[k], (str, bytes)) or not hasattr(grid[k], "__len__") or len(grid[k]) == 0:
                raise ValueError("grid[%r] must be a non-empty list of values" % (k,))
        configs = [{}]
        for k in keys:
            configs = [dict(c, **{k: v}) for c in configs for v in grid[k]]
    elif isinstance(grid, (list, tuple)) and len(grid) and all(isinstance(c, dict) for c in grid):
        configs = [dict(c) for c in grid]
    else:
        raise ValueError("grid must be None, a dict of lists or a non-empty list of dicts")
    for c in configs:
        bad = set(c) - set(GRID_JOB_KEYS) - set(GRID_SHARED_KEYS)
        if bad:
            raise ValueError("grid key %r is not one of %s" % (sorted(bad)[0], GRID_JOB_KEYS + GRID_SHARED_KEYS))
    return configs


def partition_configs(configs):
    """[(shared settings dict, [config numbers])]: the configs that agree in every GRID_SHARED_KEYS value they set can run in
    one group; the partitions come in order of first appearance."""
    parts = {}
    for i, c in enumerate(configs):
        key = tuple((k, c[k]) for k in GRID_SHARED_KEYS if k in c)
        parts.setdefault(key, []).append(i)
    return [(dict(key), members) for key, members in parts.items()]


def select_best(mean):
    """The index of the highest mean: ties go to the lowest index, a NaN mean is never best (all NaN: None)."""
    best = None
    for i, m in enumerate(mean):
        if not np.isnan(m) and (best is None or m > mean[best]):
            best = i
    return best


def cross_validate_head(emb, target, folds=5, grid=None, fold_ids=None, stratify=None, seed=0, refit=True, metric=None,
                        keep_fits=True, **settings):
    """k-fold cross-validation of a head over a grid of settings, all fits advanced together (fit_heads).
    grid: expand_grid's; a config overrides `settings` (fit_head's keywords except init / val; `seed` also seeds every fit
    unless the grid sets it).  Jobs are (config, fold): trained on the other folds, validated on the fold; configs that differ
    in a shared setting (GRID_SHARED_KEYS) run as separate groups.  fold_ids: (n,) fold numbers in [0, folds), or None for
    kfold_ids(n, folds, seed, labels) -- stratified by default for loss="ce" (stratify=True with multi-label targets is
    refused).  metric: a key of the validation record (default "mAP" for bce, "accuracy" for ce).
    -> CrossValidation(configs, fold_ids, metric, scores (configs, folds) float64, mean, std, best, fits, final): best =
    select_best(mean); fits[c][f] the HeadFit of (config, fold), None with keep_fits=False; final = fit_head on all rows with
    configs[best] when refit (else None) -- the head to use."""
    loss = settings.get("loss", "bce")
    bad = set(settings) - {"epochs", "batch_size", "lr", "betas", "eps", "weight_decay", "amsgrad", "decoupled", "shuffle",
                           "drop_last", "loss", "label_smoothing", "classes"}
    if bad:
        raise ValueError("cross_validate_head takes no setting %r" % (sorted(bad)[0],))
    ce, _ = _check_loss(loss, settings.get("label_smoothing", 0.0), settings.get("classes"))
    _check_emb(emb, device=False)
    n = int(emb.shape[0])
    configs = []
    for c in expand_grid(grid):
        full = {"seed": seed}
        full.update(settings)
        full.update(c)
        configs.append(full)
    if metric is None:
        metric = "accuracy" if ce else "mAP"
    if stratify is None:
        stratify = ce
    if fold_ids is None:
        labels = None
        if stratify:
            if not ce:
                raise ValueError("stratify=True needs single-label targets (loss=\"ce\"): multi-label rows have no one class")
            labels = labels_of(target, n, settings.get("classes"))[0]
        fold_ids = kfold_ids(n, folds, seed, labels)
    else:
        fold_ids = torch.as_tensor(fold_ids).cpu()
        if fold_ids.dim() != 1 or fold_ids.shape[0] != n or fold_ids.dtype.is_floating_point:
            raise ValueError("fold_ids must be (%d,) integers" % n)
        fold_ids = fold_ids.to(torch.int64)
        if isinstance(folds, bool) or not isinstance(folds, int) or folds < 2:
            raise ValueError("folds must be an integer >= 2 (got %r)" % (folds,))
        if int(fold_ids.min()) < 0 or int(fold_ids.max()) >= folds:
            raise ValueError("fold_ids holds values outside [0, %d)" % folds)
        if len(torch.unique(fold_ids)) != folds:
            raise ValueError("fold_ids leaves a fold empty")
    held = [torch.nonzero(fold_ids == f).reshape(-1) for f in range(folds)]
    train = [torch.nonzero(fold_ids != f).reshape(-1) for f in range(folds)]

    shared_names = ("epochs", "batch_size", "loss", "label_smoothing", "classes", "amsgrad", "decoupled", "shuffle", "drop_last")
    fits = [None] * len(configs)
    for _, members in partition_configs(configs):
        shared = {k: configs[members[0]][k] for k in shared_names if k in configs[members[0]]}
        jobs = [dict({k: configs[c][k] for k in GRID_JOB_KEYS if k in configs[c]}, rows=train[f], val=held[f])
                for c in members for f in range(folds)]
        got = fit_heads(emb, target, jobs, **shared)
        for i, c in enumerate(members):
            fits[c] = got[i * folds:(i + 1) * folds]
    scores = np.full((len(configs), folds), np.nan, dtype=np.float64)
    for c, per_fold in enumerate(fits):
        for f, fit in enumerate(per_fold):
            rec = fit.history[-1] if fit.history else {}
            if metric not in rec:
                raise ValueError("metric %r is not in the validation record (%s)" % (metric, sorted(set(rec) - {"epoch", "loss"})))
            scores[c, f] = float(rec[metric])
    mean, std = scores.mean(axis=1), scores.std(axis=1)
    best = select_best(mean)
    final = None
    if refit and best is not None:
        final = fit_head(emb, target, **configs[best])
    return CrossValidation(configs, fold_ids, metric, scores, mean, std, best, fits if keep_fits else None, final)


# ---- sound event detection heads from clip-level labels: multiple-instance learning over segments -----------------------------
# fit_head trains on scene embeddings (the mean over the clip, then LayerNorm); detect_events reads the head on every 0.32 s
# segment embedding and pools over time.  fit_sed_head trains along the path inference takes -- the reference's decision-level
# recipe (pytorch/models.py:5757-5771: head per segment, sigmoid, pooling over time; losses.py clip_bce: F.binary_cross_entropy on
# the pooled clip probability): a clip is a bag, its segments are the instances, the label belongs to the bag
# (acx_head_fit_step_mil in include/acx.h: logits, bag pass, update -- three launches per step).
MIL_POOLS = {"max": 0, "mean": 1, "linear": 2, "exp": 3}                   # enum acx_mil_pool
SedSchedule = namedtuple("SedSchedule", ["bag_idx", "bag_off", "seg_idx", "steps"])
MilGrad = namedtuple("MilGrad", ["P", "G", "loss", "terms", "tstar"])


def check_pooling(pooling):
    if pooling not in MIL_POOLS:
        raise ValueError("pooling must be one of %s (got %r)" % (", ".join("\"%s\"" % k for k in MIL_POOLS), pooling))
    return MIL_POOLS[pooling]


def _check_lengths(lengths, rows, name="segments"):
    lens = [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
    if len(lens) < 1:
        raise ValueError("%s holds no clips" % name)
    if any(v < 1 for v in lens):
        raise ValueError("%s: every clip needs at least one segment (clip %d has %d)"
                         % (name, next(i for i, v in enumerate(lens) if v < 1), min(lens)))
    if sum(lens) != rows:
        raise ValueError("%s: lengths sum to %d rows but the packed tensor holds %d" % (name, sum(lens), rows))
    return lens


def check_segments(segments, name="segments", device=True):
    """The segment embeddings of a weak-label fit in any of their three forms -- a (B, S, 768) tensor, a list of (S_i, 768)
    tensors, or (packed (M, 768), lengths) -- as (packed (M, 768) in a layout the kernels take, [S_0, S_1, ...]).  The rules
    of the rows are fit_head's (_check_emb): float32, 768 wide and, with device=True, on the GPU."""
    if isinstance(segments, torch.Tensor):
        if segments.dim() != 3 or segments.shape[2] != EMBED_DIM:
            raise ValueError("%s must be a (B, S, %d) tensor, a list of (S_i, %d) tensors or (packed, lengths) (got shape %s)"
                             % (name, EMBED_DIM, EMBED_DIM, tuple(segments.shape)))
        if segments.shape[0] < 1 or segments.shape[1] < 1:
            raise ValueError("%s holds no rows" % name)
        lens = [int(segments.shape[1])] * int(segments.shape[0])
        packed = segments.reshape(-1, EMBED_DIM)
    elif (isinstance(segments, tuple) and len(segments) == 2 and isinstance(segments[0], torch.Tensor)
          and not (isinstance(segments[1], torch.Tensor) and segments[1].dim() == 2)):
        packed = segments[0]
        if packed.dim() != 2:
            raise ValueError("%s: the packed tensor must be (M, %d) (got shape %s)" % (name, EMBED_DIM, tuple(packed.shape)))
        lens = _check_lengths(segments[1], int(packed.shape[0]), name)
    elif isinstance(segments, (list, tuple)) and len(segments) and all(isinstance(s, torch.Tensor) for s in segments):
        for i, s in enumerate(segments):
            if s.dim() != 2 or s.shape[1] != EMBED_DIM or s.dtype != segments[0].dtype or s.device != segments[0].device:
                raise ValueError("%s[%d] must be a (S_i, %d) tensor of the dtype and device of %s[0] (got %s, %s, %s)"
                                 % (name, i, EMBED_DIM, name, tuple(s.shape), s.dtype, s.device))
        lens = _check_lengths([s.shape[0] for s in segments], sum(int(s.shape[0]) for s in segments), name)
        packed = torch.cat(list(segments))
    else:
        raise ValueError("%s must be a (B, S, %d) tensor, a list of (S_i, %d) tensors or (packed, lengths) (got %s)"
                         % (name, EMBED_DIM, EMBED_DIM, type(segments).__name__))
    return _check_emb(packed, name, device), lens


def sed_schedule(lengths, epochs, batch_size, seed=0, shuffle=True, drop_last=False):
    """The index arrays of every step of a weak-label fit, built once (acx_head_fit_step_mil's bag_idx / bag_off / seg_idx):
    clip i owns the rows [sum(lengths[:i]), sum(lengths[:i + 1])) of the packed embeddings; epoch e visits the clips in
    epoch_orders(n, epochs, seed, shuffle)[e], cut into epoch_batches(n, batch_size, drop_last).  -> SedSchedule of three numpy
    arrays, each the steps' own arrays laid back to back -- bag_idx int64 (the clips of the batch), bag_off int32 (bags + 1
    entries per step, from 0 to the step's seg_rows), seg_idx int64 (the rows of the batch's segments, in bag order) -- and
    steps: one (bag_start, bags, off_start, seg_start, seg_rows) per step, the places of its slices in them."""
    lens = np.asarray(lengths, dtype=np.int64)
    n = int(lens.shape[0])
    first = np.concatenate([[0], np.cumsum(lens)])[:-1]
    order = epoch_orders(n, epochs, seed, shuffle).numpy()
    batches = epoch_batches(n, batch_size, drop_last)
    used = sum(rows for _, rows in batches)
    bag_idx, bag_off, seg_idx, steps = [], [], [], []
    nb = no = ns = 0
    for e in range(int(epochs)):                                   # an epoch at a time: its steps are slices of these arrays
        b = order[e, :used]
        l = lens[b]
        cum = np.concatenate([[0], np.cumsum(l)])
        bag_idx.append(b)
        seg_idx.append(np.repeat(first[b] - cum[:-1], l) + np.arange(cum[-1], dtype=np.int64))
        for start, rows in batches:
            bag_off.append(cum[start:start + rows + 1] - cum[start])
            seg_rows = int(cum[start + rows] - cum[start])
            steps.append((nb, rows, no, ns, seg_rows))
            nb, no, ns = nb + rows, no + rows + 1, ns + seg_rows
    cat = lambda parts, dt: np.concatenate(parts).astype(dt, copy=False) if parts else np.zeros(0, dtype=dt)       # noqa: E731
    return SedSchedule(cat(bag_idx, np.int64), cat(bag_off, np.int32), cat(seg_idx, np.int64), steps)


def _padded_bags(z, bag_off):
    """z (rows, N) with bag i in rows [bag_off[i], bag_off[i + 1]) -> (zb (bags, Smax, N), mask (bags, Smax), lens (bags,))."""
    off = torch.as_tensor(np.asarray(bag_off, dtype=np.int64))
    if off.dim() != 1 or off.shape[0] < 2 or int(off[0]) != 0 or bool((off[1:] < off[:-1]).any()) or int(off[-1]) != z.shape[0]:
        raise ValueError("bag_off must run from 0 to the %d rows of z without decreasing" % z.shape[0])
    lens = off[1:] - off[:-1]
    smax = max(int(lens.max()), 1)
    ar = torch.arange(smax)
    mask = ar[None, :] < lens[:, None]
    rows = (off[:-1, None] + ar[None, :]).clamp(max=max(z.shape[0] - 1, 0))
    zb = z[rows] if z.shape[0] else z.new_zeros((lens.shape[0], smax, z.shape[1]))
    return torch.where(mask[:, :, None], zb, torch.zeros_like(zb)), mask, lens


def mil_forward_host(z, bag_off, pooling):
    """The pooled clip probabilities of segment logits, in torch ops of z's dtype (float64 for the definition), differentiable:
    q = sigmoid(z) per segment, then over the S rows of a bag
        "max"     P = q at t*, the LOWEST t that attains max_t z_t (taken on the logits)
        "mean"    P = sum q / S
        "linear"  P = sum q^2 / sum q   (sum q = 0: P = 0)
        "exp"     P = sum q e^q / sum e^q
    and P = 0 for an empty bag.  -> (P (bags, N), tstar (bags, N) int64: t* within the bag, for "max"; else None)."""
    check_pooling(pooling)
    zb, mask, lens = _padded_bags(z, bag_off)
    m3 = mask[:, :, None]
    some = (lens > 0)[:, None]
    q = torch.sigmoid(zb)
    zero = torch.zeros((), dtype=z.dtype)
    tstar = None
    if pooling == "max":
        zm = torch.where(m3, zb.detach(), torch.full_like(zb, float("-inf")))
        top = zm.max(dim=1).values
        ar = torch.arange(zb.shape[1])[None, :, None].expand_as(zm)
        tstar = torch.where((zm == top[:, None, :]) & m3, ar, torch.full_like(ar, zb.shape[1] - 1)).min(dim=1).values
        P = torch.where(some, q.gather(1, tstar[:, None, :]).squeeze(1), zero)
    elif pooling == "mean":
        P = torch.where(m3, q, zero).sum(dim=1) / lens.clamp(min=1)[:, None].to(z.dtype)
    elif pooling == "linear":
        qm = torch.where(m3, q, zero)
        s1 = qm.sum(dim=1)
        P = (qm * qm).sum(dim=1) / torch.where(s1 == 0, torch.ones_like(s1), s1)
    else:
        e = torch.where(m3, torch.exp(q), zero)
        P = (q * e).sum(dim=1) / torch.where(some, e.sum(dim=1), torch.ones((), dtype=z.dtype))
    return P, tstar


def mil_grad_host(z, bag_off, y, pooling, dtype=torch.float64):
    """One bag pass in float64 (or `dtype`), in closed form: z (rows, N) segment logits, bag i in rows [bag_off[i], bag_off[i + 1]), y
    (bags, N) clip labels in [0, 1].  P = mil_forward_host(z); per (bag, class)
        term  = -[y max(log P, -100) + (1 - y) max(log1p(-P), -100)],  loss = mean(term)
        dL/dP = (P - y) / max(P (1 - P), 1e-12)                          -- F.binary_cross_entropy and its backward
        dP/dq = [t = t*] | 1 / S | (2 q - P) / sum q | e^q (1 + q - P) / sum e^q   ("linear" with sum q = 0: 0)
        G[t]  = dL/dP dP/dq_t q_t (1 - q_t) / (bags N)
    -> MilGrad(P, G (rows, N), loss, terms (bags, N), tstar).  Autograd through mil_forward_host and F.binary_cross_entropy
    gives the same G (tests/test_sed_fit_cpu.py)."""
    z = torch.as_tensor(z).detach().to(dtype)
    y = torch.as_tensor(y).detach().to(dtype)
    P, tstar = mil_forward_host(z, bag_off, pooling)
    zb, mask, lens = _padded_bags(z, bag_off)
    if tuple(y.shape) != tuple(P.shape):
        raise ValueError("y must be (%d, %d) (got %s)" % (P.shape[0], P.shape[1], tuple(y.shape)))
    m3 = mask[:, :, None]
    q = torch.sigmoid(zb)
    terms = -(y * torch.log(P).clamp(min=-100) + (1 - y) * torch.log1p(-P).clamp(min=-100))
    dLdP = ((P - y) / (P * (1 - P)).clamp(min=1e-12))[:, None, :]
    P3 = P[:, None, :]
    if pooling == "max":
        d = (torch.arange(zb.shape[1])[None, :, None] == tstar[:, None, :]).to(dtype)
    elif pooling == "mean":
        d = (1.0 / lens.clamp(min=1).to(dtype))[:, None, None].expand_as(q)
    elif pooling == "linear":
        s1 = torch.where(m3, q, torch.zeros_like(q)).sum(dim=1, keepdim=True)
        d = torch.where(s1 == 0, torch.zeros_like(q), (2 * q - P3) / torch.where(s1 == 0, torch.ones_like(s1), s1))
    else:
        e = torch.exp(q)
        s1 = torch.where(m3, e, torch.zeros_like(e)).sum(dim=1, keepdim=True)
        d = e * (1 + q - P3) / torch.where(s1 == 0, torch.ones_like(s1), s1)
    G = dLdP * d * (q * (1 - q)) / (P.shape[0] * P.shape[1])
    return MilGrad(P, G[mask], terms.mean(), terms, tstar)


def fit_sed_head_host(segments, target, pooling="max", epochs=20, batch_size=64, lr=1e-4, betas=(0.9, 0.999), eps=1e-8,
                      weight_decay=0.0, amsgrad=True, decoupled=False, init=None, seed=0, shuffle=True, drop_last=False,
                      dtype=torch.float64, on_step=None, closed_form=False):
    """fit_sed_head's definition on the CPU: the same schedule (sed_schedule), the same initial head, then per step autograd
    through sigmoid -> mil_forward_host -> F.binary_cross_entropy and torch.optim.Adam / AdamW, in `dtype`.
    closed_form: the gradients come from mil_grad_host in `dtype` (G, then G^T E and its column sums) instead of autograd -- the
    same definition, evaluated in another order.  on_step(t, z, bag_off, E[seg_idx], W, b): called with every step's logits and inputs before the update (tests read margins).
    -> HeadFit(weight, bias, loss (steps,), [])."""
    check_pooling(pooling)
    _check_hyper(epochs, batch_size, betas, eps, weight_decay)
    packed, lens = check_segments(segments, device=False)
    target = torch.as_tensor(target)
    if target.dim() != 2 or target.shape[0] != len(lens):
        raise ValueError("target must be a (%d, N) tensor (got %s)" % (len(lens), tuple(target.shape)))
    N = int(target.shape[1])
    w0, b0 = init_head(N, seed) if init is None else _check_init(init, N)
    E, Y = packed.detach().cpu().to(dtype), target.detach().cpu().to(dtype)
    W = w0.detach().cpu().to(dtype).clone().requires_grad_()
    b = b0.detach().cpu().to(dtype).clone().requires_grad_()
    sched = sed_schedule(lens, epochs, batch_size, seed, shuffle, drop_last)
    lrs = _lr_schedule(lr, len(sched.steps))
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([W, b], lr=lrs[0] if lrs else 0.0, betas=tuple(betas), eps=eps,
                                                                  weight_decay=weight_decay, amsgrad=amsgrad)
    losses = []
    for t, (nb, bags, no, ns, rows) in enumerate(sched.steps):
        opt.param_groups[0]["lr"] = lrs[t]
        e = E[torch.from_numpy(sched.seg_idx[ns:ns + rows])]
        z = e @ W.T + b
        if on_step is not None:
            on_step(t, z.detach(), sched.bag_off[no:no + bags + 1].tolist(), e, W.detach().clone(), b.detach().clone())
        yb = Y[torch.from_numpy(sched.bag_idx[nb:nb + bags])]
        if closed_form:
            g = mil_grad_host(z, sched.bag_off[no:no + bags + 1], yb, pooling, dtype=dtype)
            loss, W.grad, b.grad = g.loss, g.G.T @ e, g.G.sum(dim=0)
        else:
            P, _ = mil_forward_host(z, sched.bag_off[no:no + bags + 1], pooling)
            loss = torch.nn.functional.binary_cross_entropy(P, yb)
            opt.zero_grad()
            loss.backward()
        opt.step()
        losses.append(loss.detach())
    return HeadFit(W.detach(), b.detach(), torch.stack(losses) if losses else torch.zeros(0, dtype=dtype), [])


def _validate_sed(weight, bias, seg_val, lens_val, target_val, pooling):
    from .metrics import tagging_metrics
    from .segments import pool_segments
    probs = pool_segments(torch.addmm(bias, seg_val, weight.t()), pooling, steps=lens_val)
    stats = tagging_metrics(target_val, probs)
    return {"average_precision": stats["average_precision"], "auc": stats["auc"], "d_prime": stats["d_prime"],
            "mAP": float(np.mean(stats["average_precision"])), "mAUC": float(np.nanmean(stats["auc"]))}


def fit_sed_head(segments, target, pooling="max", epochs=20, batch_size=64, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 amsgrad=True, decoupled=False, init=None, seed=0, shuffle=True, drop_last=False, val=None):
    """Train an nn.Linear(768, N) sound event detection head from CLIP-level labels: the head is applied to every segment
    embedding of a clip, the segment probabilities are pooled over time (`pooling`: "max", the pooling forward_segments'
    "clipwise_output" and detect_events use; "mean", "linear" or "exp", read at inference with segments.pool_segments) and
    F.binary_cross_entropy is taken on the pooled clip probability -- multiple-instance learning, on the GPU
    (acx_head_fit_step_mil: three launches per step, nothing synchronises).
    segments: (B, S, 768), a list of (S_i, 768), or (packed (M, 768), lengths) -- forward_segment_embeddings /
    extract(what="segment_embeddings") outputs; target: (clips, N) bool / uint8 / float, fit_head's rules; batch_size counts
    clips.  The other settings, the epoch order and the initial head are fit_head's.  val=(segments_val, target_val):
    per-epoch tagging_metrics of the POOLED clip probabilities in the history (one synchronisation per epoch).
    Returns HeadFit(weight, bias, loss, history)."""
    pool = check_pooling(pooling)
    _check_hyper(epochs, batch_size, betas, eps, weight_decay)
    emb, lens = check_segments(segments)
    n, device, rows_total = len(lens), emb.device, int(emb.shape[0])
    tgt = _check_target(target, n, device, "segments")
    N = int(tgt.shape[1])
    if val is not None:
        if len(val) != 2:
            raise ValueError("val must be (segments_val, target_val)")
        seg_val, lens_val = check_segments(val[0], "segments_val")
        if seg_val.device != device:
            raise ValueError("segments_val is on %s, segments on %s" % (seg_val.device, device))
        target_val = _check_target(val[1], len(lens_val), device, "segments_val", "target_val")
        if target_val.shape[1] != N:
            raise ValueError("target_val has %d classes, target %d" % (target_val.shape[1], N))
    w0, b0 = init_head(N, seed) if init is None else _check_init(init, N)
    sched = sed_schedule(lens, epochs, batch_size, seed, shuffle, drop_last)
    steps = len(sched.steps)
    lrs = _lr_schedule(lr, steps)
    seg_max = max((s[4] for s in sched.steps), default=1)
    if seg_max > _ffi.FIT_MAX_ROWS:
        raise ValueError("a batch of %d clips holds %d segments (at most 2^22 per step): lower batch_size" % (batch_size, seg_max))

    with torch.no_grad(), torch.cuda.device(device):
        W = w0.detach().to(device=device, dtype=torch.float32, copy=True).contiguous()
        b = b0.detach().to(device=device, dtype=torch.float32, copy=True).contiguous()
        loss = torch.zeros(steps, dtype=torch.float32, device=device)
        history = []
        if steps == 0:
            return HeadFit(W, b, loss, history)
        bag_idx, bag_off, seg_idx = (torch.from_numpy(a).to(device) for a in (sched.bag_idx, sched.bag_off, sched.seg_idx))
        mom = torch.zeros((3, N, EMBED_DIM), dtype=torch.float32, device=device)
        momb = torch.zeros((3, N), dtype=torch.float32, device=device)
        status = torch.zeros(1, dtype=torch.int32, device=device)
        ws_bytes = _ffi.head_fit_mil_workspace_bytes(seg_max, min(batch_size, n), N)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        step_fn = _ffi.lib().acx_head_fit_step_mil
        hp = _ffi.adam(betas[0], betas[1], eps, weight_decay, amsgrad, decoupled)
        fixed_a = (vp(emb), emb.stride(0), rows_total, vp(tgt), _inputs.target_code(tgt), tgt.stride(0), n)
        fixed_b = (N, pool, vp(W), vp(b), vp(mom[0]), vp(mom[1]), vp(mom[2]) if amsgrad else None, vp(momb[0]), vp(momb[1]),
                   vp(momb[2]) if amsgrad else None, ctypes.byref(hp))
        tail = (vp(status), vp(ws), ws_bytes, _ffi.stream_ptr(device))
        bi, bo, si, loss_ptr = bag_idx.data_ptr(), bag_off.data_ptr(), seg_idx.data_ptr(), loss.data_ptr()
        per = steps // epochs
        for t, (nb, bags, no, ns, rows) in enumerate(sched.steps):
            rc = step_fn(*fixed_a, ctypes.c_void_p(si + 8 * ns), rows, ctypes.c_void_p(bo + 4 * no), ctypes.c_void_p(bi + 8 * nb),
                         bags, *fixed_b, t + 1, lrs[t], ctypes.c_void_p(loss_ptr + 4 * t), *tail)
            if rc != _ffi.OK:
                _ffi.check(rc)
            if (t + 1) % per == 0:
                e = t // per
                rec = {"epoch": e, "loss": loss[e * per:(e + 1) * per].mean()}
                if val is not None:
                    rec.update(_validate_sed(W, b, seg_val, lens_val, target_val, pooling))
                history.append(rec)
    return HeadFit(W, b, loss, history)
