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
    if not isinstance(target, torch.Tensor) or target.dim() != 2 or target.shape[0] != emb.shape[0]:
        raise ValueError("%s must be a (%d, N) tensor (got %s)" % (tname, emb.shape[0], getattr(target, "shape", type(target))))
    if target.device != emb.device:
        raise ValueError("%s is on %s, %s on %s" % (tname, target.device, name, emb.device))
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
    t = _inputs.rows(t)
    return emb, t, _inputs.target_code(t)


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
    _check_hyper(epochs, batch_size, betas, eps, weight_decay)
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
        if len(init) != 2:
            raise ValueError("init must be (weight, bias)")
        w0, b0 = init
        if tuple(w0.shape) != (N, EMBED_DIM) or tuple(b0.shape) != (N,):
            raise ValueError("init must be a (%d, %d) weight and a (%d,) bias (got %s and %s)"
                             % (N, EMBED_DIM, N, tuple(w0.shape), tuple(b0.shape)))
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
