#!/usr/bin/env python
"""Fine-tune a classifier head on this backbone -- counterpart of the reference's pytorch/finetune_audiocaps.py with the base
frozen: scene embeddings are extracted once, the head is fitted on them on the GPU (ConvNeXt.fit_head), and the result is saved
as a checkpoint that ConvNeXt.from_pretrained loads as an N-class model.

    python demo_finetune.py --ckpt checkpoints/model.safetensors --data sounds/ --out my_tagger/        # sounds/<class>/*.wav
    python demo_finetune.py --ckpt ... --csv clips.csv --out my_tagger/        # lines: path.wav,label[;label...]
    python demo_finetune.py --synthetic --out /tmp/tagger                      # seeded weights and clips, no files needed
    python demo_finetune.py --ckpt ... --data sounds/ --loss ce --out my_classifier/    # one class per clip: softmax cross-entropy
    python demo_finetune.py --ckpt ... --data sounds/ --loss ce --folds 5 --grid-lr 1e-4,3e-4,1e-3 --out my_classifier/

Writes <out>/model.safetensors, <out>/model.pth ({"model": state_dict}) and <out>/labels.txt (one class name per line, in head
order).  With a validation split, one decision threshold per class is chosen on it (the largest F1, metrics.operating_points)
and written next to <out> as <out>.thresholds.npy -- demo_convnext.py --thresholds takes it.  16-bit PCM WAV files at any rate
(resampled on the device).  --loss ce trains a single-label head (every clip needs exactly one label): it prints validation
accuracy, top-5 accuracy and the five largest confusions, and writes no thresholds file -- read the model with
ConvNeXt.classify / demo_convnext.py --softmax.  With a validation split the head's probabilities are also calibrated on it
(pytorch/calibration.py: per-class Platt scaling for --loss bce, temperature scaling for --loss ce): the ECE before and after is
printed and the map written as <out>.calibration.npz -- demo_convnext.py --calibration takes it.
--folds K cross-validates the settings of --grid-lr x --grid-weight-decay (default: the one --lr / --weight-decay pair) on the
training split first, all K x settings fits advanced together on the GPU (ConvNeXt.cross_validate_head): one line per setting,
the best marked; the run then continues as above with the best setting.
--augment reference fits the head as the reference fine-tunes -- on augmented views of the training clips instead of their
plain embeddings (ConvNeXt.forward_augmented: SpecAugment stripes; "full" adds gain, roll and speed perturbation), --views K
passes over them, --mixup-alpha A mixing clips and label rows pairwise (--loss bce).  The clips must share one length; validation,
thresholds and calibration stay on the plain embeddings.

    python demo_finetune.py --synthetic --augment reference --views 4 --mixup-alpha 0.5 --out /tmp/tagger

--sed-pooling max|mean|linear|exp fits a sound event detection head from the same clip labels instead (ConvNeXt.fit_sed_head):
the head is trained on every clip's 0.32 s segment embeddings through that pooling over time -- the path detect_events and
psds read it on -- and the validation mAP is taken of the pooled clip probabilities.  Without the flag nothing changes.

    python demo_finetune.py --synthetic --sed-pooling linear --lr 1e-3 --out /tmp/detector"""
import argparse
import csv
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from audioset_convnext_inf_amd.pytorch.convnext import ConvNeXt, convnext_tiny      # noqa: E402
from audioset_convnext_inf_amd.pytorch.extract_embeddings import extract            # noqa: E402
from audioset_convnext_inf_amd.utils.utilities import read_wav_pcm16                # noqa: E402


def folder_items(root):
    """[(path, [class])] of root/<class>/*.wav"""
    items = []
    for cls in sorted(os.listdir(root)):
        d = os.path.join(root, cls)
        if os.path.isdir(d):
            items += [(os.path.join(d, f), [cls]) for f in sorted(os.listdir(d)) if f.lower().endswith(".wav")]
    return items


def csv_items(path):
    """[(path, [labels])] of lines `file.wav,label;label` (paths relative to the CSV's folder)"""
    base = os.path.dirname(os.path.abspath(path))
    with open(path, newline="") as f:
        return [(os.path.join(base, r[0]), [s.strip() for s in r[1].split(";") if s.strip()])
                for r in csv.reader(f) if len(r) >= 2 and r[0].lower().endswith(".wav")]


def synthetic_items(clips, classes, seconds, seed=0):
    """Seeded clips whose class decides a tone mixed into noise -> (waveforms, (clips, classes) bool targets, names)"""
    g = torch.Generator().manual_seed(seed)
    label = torch.randint(0, classes, (clips,), generator=g)
    t = torch.arange(int(seconds * 32000)) / 32000.0
    waves = [0.1 * torch.randn(t.numel(), generator=g) + 0.3 * torch.sin(2 * torch.pi * (200.0 + 150.0 * int(c)) * t) for c in label]
    target = torch.zeros(clips, classes, dtype=torch.bool)
    target[torch.arange(clips), label] = True
    return waves, target, ["tone_%d" % c for c in range(classes)]


def sed_fit(model, waves, target, names, rate, a):
    """--sed-pooling: the weak-label SED fit.  Segment embeddings of every clip, the head trained through the pooling over time
    on the clip labels (the path detect_events takes), validation mAP of the pooled clip probabilities per epoch."""
    if a.loss != "bce" or a.folds or a.augment:
        sys.exit("--sed-pooling fits with binary cross-entropy on the clips as they are: no --loss ce, --folds or --augment")
    t0 = time.perf_counter()
    with torch.no_grad():
        segs = []
        for s in range(0, len(waves), 256):
            part = model.forward_varlen([torch.as_tensor(w, dtype=torch.float32).cuda() for w in waves[s:s + 256]],
                                        what="segment_embeddings", sample_rate=rate)
            segs += [p.clone() for p in part]
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    n_val = int(len(waves) * a.val_fraction) if len(waves) >= 20 else 0
    order = torch.randperm(len(waves), generator=torch.Generator().manual_seed(a.seed)).tolist()
    tr, va = order[n_val:], order[:n_val]
    target = target.cuda()
    pick = lambda rows: ([segs[i] for i in rows], target[torch.tensor(rows, device="cuda")])       # noqa: E731
    fit = model.fit_sed_head(*pick(tr), pooling=a.sed_pooling, epochs=a.epochs, batch_size=a.batch_size, lr=a.lr,
                             weight_decay=a.weight_decay, decoupled=a.adamw, seed=a.seed, val=pick(va) if n_val else None)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    for rec in fit.history:
        print("epoch %2d  loss %.4f%s" % (rec["epoch"], float(rec["loss"]),
                                          "  val mAP %.3f  AUC %.3f (clip probabilities pooled with %s)" % (rec["mAP"], rec["mAUC"], a.sed_pooling)
                                          if n_val else ""))
    print("segment embeddings %.2f s (%d segments of %d clips), fit %.2f s (%d steps%s)"
          % (t1 - t0, sum(s.shape[0] for s in segs), len(waves), t2 - t1, fit.loss.numel(), ", validation included" if n_val else ""))
    os.makedirs(a.out, exist_ok=True)
    sd = {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}
    torch.save({"model": sd}, os.path.join(a.out, "model.pth"))
    from safetensors.torch import save_file
    save_file(sd, os.path.join(a.out, "model.safetensors"))
    with open(os.path.join(a.out, "labels.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    print("wrote %s: model.safetensors, model.pth, labels.txt -- a %d-class head for detect_events / psds%s"
          % (a.out, len(names), "" if a.sed_pooling == "max" else
             "; clip probabilities: segments.pool_segments(segmentwise_logits, %r)" % a.sed_pooling))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", default="topel/ConvNeXt-Tiny-AT", help="local .safetensors/.pth, Zenodo URL or HF model id")
    ap.add_argument("--data", help="folder with one sub-folder of .wav files per class")
    ap.add_argument("--csv", help="CSV of `path.wav,label[;label...]`")
    ap.add_argument("--synthetic", action="store_true", help="seeded synthetic weights and clips (2 000 x 1 s, 50 classes)")
    ap.add_argument("--clips", type=int, default=2000)
    ap.add_argument("--classes", type=int, default=50)
    ap.add_argument("--out", required=True)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--weight-decay", type=float, default=0.0)
    ap.add_argument("--adamw", action="store_true")
    ap.add_argument("--loss", choices=("bce", "ce"), default="bce", help="ce: softmax cross-entropy for one label per clip")
    ap.add_argument("--label-smoothing", type=float, default=0.0, help="--loss ce only")
    ap.add_argument("--val-fraction", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--folds", type=int, default=0, help="K-fold cross-validation of the grid on the training split first")
    ap.add_argument("--grid-lr", help="comma-separated learning rates for --folds (default: --lr)")
    ap.add_argument("--grid-weight-decay", help="comma-separated weight decays for --folds (default: --weight-decay)")
    ap.add_argument("--augment", choices=("reference", "full"), help="fit on augmented views of the training clips")
    ap.add_argument("--views", type=int, default=1, help="augmented passes over the training clips (--augment)")
    ap.add_argument("--mixup-alpha", type=float, help="mixup of clip pairs and their label rows (--augment, --loss bce)")
    ap.add_argument("--sed-pooling", choices=("max", "mean", "linear", "exp"),
                    help="fit a sound event detection head from the clip labels instead (ConvNeXt.fit_sed_head): the head is trained "
                         "on segment embeddings through this pooling over time")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("this build runs on an MI355X; no GPU is visible")

    rate = None
    if a.synthetic:
        from audioset_convnext_inf_amd import synth
        model = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56], use_speed_perturb=False)
        model.load_state_dict(synth.synth_state_dict(0))
        waves, target, names = synthetic_items(a.clips, a.classes, 1.0, a.seed)
    else:
        if not (a.data or a.csv):
            sys.exit("give --data, --csv or --synthetic")
        model = ConvNeXt.from_pretrained(a.ckpt, map_location="cpu")
        if model is None:
            sys.exit(1)
        items = folder_items(a.data) if a.data else csv_items(a.csv)
        if not items:
            sys.exit("no .wav files found")
        names = sorted({l for _, ls in items for l in ls})
        col = {n: i for i, n in enumerate(names)}
        waves, target = [], torch.zeros(len(items), len(names), dtype=torch.bool)
        for i, (path, labels) in enumerate(items):
            wav, sr = read_wav_pcm16(path)
            if rate is None:
                rate = sr
            elif sr != rate:
                sys.exit("%s is at %d Hz, the clips before it at %d Hz: one rate per run" % (path, sr, rate))
            waves.append(torch.from_numpy(wav[0]))
            target[i, [col[l] for l in labels]] = True
    model = model.to("cuda").eval()
    print("%d clips, %d classes" % (len(waves), len(names)))
    if a.sed_pooling:
        return sed_fit(model, waves, target, names, rate, a)

    t0 = time.perf_counter()
    emb = torch.stack(extract(model, waves, what="scene", pack=True, sample_rate=rate)).cuda()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    n_val = int(len(waves) * a.val_fraction) if len(waves) >= 20 else 0
    order = torch.randperm(len(waves), generator=torch.Generator().manual_seed(a.seed)).cuda()
    tr, va = order[n_val:], order[:n_val]
    target = target.cuda()
    ce = a.loss == "ce"
    if ce and not bool((target.sum(dim=1) == 1).all()):
        sys.exit("--loss ce needs exactly one label per clip")
    extra = dict(loss="ce", label_smoothing=a.label_smoothing) if ce else {}
    train_emb, train_target = emb[tr], target[tr]
    if a.augment:
        from audioset_convnext_inf_amd.pytorch import augment
        if ce and a.mixup_alpha is not None:
            sys.exit("--mixup-alpha gives soft label rows: use it with --loss bce")
        rows = tr.tolist()
        if a.mixup_alpha is not None and len(rows) % 2:
            rows = rows[:-1]                    # mixup pairs clips
        try:
            train_emb, train_target = augment.augmented_embeddings(
                model, [waves[i].cuda() for i in rows], target[torch.tensor(rows, device="cuda")], augment.policy_of(a.augment),
                views=a.views, mixup_alpha=a.mixup_alpha, seed=a.seed, sample_rate=rate)
        except ValueError as e:
            sys.exit("--augment: %s" % e)
        torch.cuda.synchronize()
        print("augmented views: %d rows from %d clips (%s, %d views%s) in %.2f s" % (
            train_emb.shape[0], len(rows), a.augment, a.views,
            "" if a.mixup_alpha is None else ", mixup alpha %g" % a.mixup_alpha, time.perf_counter() - t1))
        t1 = time.perf_counter()
    if a.folds:
        grid = {"lr": [float(v) for v in a.grid_lr.split(",")] if a.grid_lr else [a.lr],
                "weight_decay": [float(v) for v in a.grid_weight_decay.split(",")] if a.grid_weight_decay else [a.weight_decay]}
        cv = model.cross_validate_head(train_emb, train_target, folds=a.folds, grid=grid, seed=a.seed, refit=False, install=False,
                                       keep_fits=False, epochs=a.epochs, batch_size=a.batch_size, decoupled=a.adamw, **extra)
        torch.cuda.synchronize()
        for c, cfg in enumerate(cv.configs):
            print("%s lr %-8g weight decay %-8g  %s %.3f +- %.3f  (%s)" % (
                "*" if c == cv.best else " ", cfg["lr"], cfg["weight_decay"], cv.metric, cv.mean[c], cv.std[c],
                " ".join("%.3f" % v for v in cv.scores[c])))
        if cv.best is None:
            sys.exit("every setting's %s is NaN: no best setting" % cv.metric)
        a.lr, a.weight_decay = cv.configs[cv.best]["lr"], cv.configs[cv.best]["weight_decay"]
        print("cross-validation %.2f s (%d folds x %d settings); continuing with lr %g, weight decay %g"
              % (time.perf_counter() - t1, a.folds, len(cv.configs), a.lr, a.weight_decay))
        t1 = time.perf_counter()
    fit = model.fit_head(train_emb, train_target, epochs=a.epochs, batch_size=a.batch_size, lr=a.lr, weight_decay=a.weight_decay,
                         decoupled=a.adamw, seed=a.seed, val=(emb[va], target[va]) if n_val else None, **extra)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    for rec in fit.history:
        if ce:
            val = "  val accuracy %.3f  top-5 %.3f  macro F1 %.3f" % (rec["accuracy"], rec["topk_accuracy"], rec["macro_f1"]) if n_val else ""
        else:
            val = "  val mAP %.3f  AUC %.3f" % (rec["mAP"], rec["mAUC"]) if n_val else ""
        print("epoch %2d  loss %.4f%s" % (rec["epoch"], float(rec["loss"]), val))
    print("extraction %.2f s (%.0f clips/s), fit %.2f s (%d steps%s)" % (t1 - t0, len(waves) / (t1 - t0), t2 - t1, fit.loss.numel(),
                                                                           ", validation included" if n_val else ""))

    thresholds = None
    calibration = None
    if n_val and ce:
        from audioset_convnext_inf_amd.pytorch import calibration as cal
        from audioset_convnext_inf_amd.pytorch.classify import classification_metrics
        head = model.head_audioset
        with torch.no_grad():
            val_labels = target[va].int().argmax(dim=1)
            val_logits = torch.addmm(head.bias, emb[va], head.weight.t())
            m = classification_metrics(val_labels, val_logits, k=5, confusion=len(names) <= 4096)
            calibration = cal.fit_temperature(val_labels, val_logits)
            before = cal.reliability_toplabel(val_labels, val_logits)
            after = cal.reliability_toplabel(val_labels, val_logits, calibration=calibration)
        note = {cal.NOT_CONVERGED: " (not converged)", cal.AT_BOUND: " (at a bound)", cal.DEGENERATE: " (constant rows)"}
        print("temperature scaling: T = %.3f%s  top-label ECE before %.4f  after %.4f  (NLL %.4f -> %.4f)"
              % (calibration.temperature, note.get(int(calibration.info.item()), ""), before.ece, after.ece, before.nll, after.nll))
        print("val accuracy %.3f  top-%d accuracy %.3f  balanced accuracy %.3f  macro F1 %.3f  (%d clips)"
              % (m.accuracy, m.k, m.topk_accuracy, m.balanced_accuracy, m.macro_f1, m.counted))
        if m.confusion is not None:
            conf = m.confusion.cpu().numpy().copy()
            np.fill_diagonal(conf, 0)
            for flat in np.argsort(conf, axis=None)[::-1][:5]:
                t, p = divmod(int(flat), len(names))
                if conf[t, p]:
                    print("    %d x %s taken for %s" % (conf[t, p], names[t], names[p]))
    elif n_val:
        # one threshold per class, chosen where the labels are: the largest F1 on the validation split
        import warnings
        from audioset_convnext_inf_amd.pytorch.metrics import operating_points
        head = model.head_audioset
        from audioset_convnext_inf_amd.pytorch import calibration as cal
        with torch.no_grad():
            val_logits = torch.addmm(head.bias, emb[va], head.weight.t())
            probs = torch.sigmoid(val_logits)
            calibration = cal.fit_platt(target[va], val_logits)
            before = cal.reliability(target[va], probs)
            after = cal.reliability(target[va], calibration.apply(val_logits))
        info = calibration.info.cpu().numpy()
        print("Platt scaling: class-wise ECE before %.4f  after %.4f  (Brier %.4f -> %.4f; %d of %d classes kept the identity, "
              "%d did not converge)" % (before.classwise_ece, after.classwise_ece, before.brier.mean(), after.brier.mean(),
                                        int((info == cal.DEGENERATE).sum()), len(names), int((info == cal.NOT_CONVERGED).sum())))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)          # classes the split holds no positive of: counted below
            op = operating_points(target[va], probs, criterion="f1")
        thresholds = op.threshold.cpu().numpy()
        print("val F1 at per-class thresholds: macro %.3f  micro %.3f  (mAP %.3f; %d of %d classes without a positive never fire)"
              % (op.macro()["f"], op.micro()["f"], fit.history[-1]["mAP"], int(np.isinf(thresholds).sum()), len(names)))
        # the per-clip view of the same scores: what multi-label benchmarks outside AudioSet report (lwlrap: DCASE 2019 Task 2)
        from audioset_convnext_inf_amd.pytorch.ranking import ranking_metrics
        rank = ranking_metrics(target[va], probs)
        print("val lwlrap %.3f  LRAP %.3f  (coverage error %.2f, ranking loss %.4f)"
              % (rank.lwlrap, rank.lrap, rank.coverage_error, rank.ranking_loss))

    os.makedirs(a.out, exist_ok=True)
    sd = {k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}
    torch.save({"model": sd}, os.path.join(a.out, "model.pth"))
    from safetensors.torch import save_file
    save_file(sd, os.path.join(a.out, "model.safetensors"))
    with open(os.path.join(a.out, "labels.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    if thresholds is not None:
        thr_path = a.out.rstrip("/" + os.sep) + ".thresholds.npy"
        np.save(thr_path, thresholds)
        print("wrote %s: %d per-class thresholds (demo_convnext.py --thresholds)" % (thr_path, len(thresholds)))
    if calibration is not None:
        cal_path = a.out.rstrip("/" + os.sep) + ".calibration.npz"
        calibration.save(cal_path)
        print("wrote %s: the %s map fitted on the validation split (demo_convnext.py --calibration)"
              % (cal_path, "temperature" if ce else "Platt"))
    print("wrote %s: model.safetensors, model.pth, labels.txt -- ConvNeXt.from_pretrained(%r) loads it as a %d-class model"
          % (a.out, os.path.join(a.out, "model.safetensors"), len(names)))


if __name__ == "__main__":
    main()
