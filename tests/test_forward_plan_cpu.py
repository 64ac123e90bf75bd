"""CPU: the workspace plan of every forward, as data (acx_test_forward_plan: host arithmetic, no context, no device).

A forward carves its workspace into regions -- feat, x of the four stages, and y / hidden / stats sized for one block of stage 0 --
and lends them to tenants they were not sized for (the dense-DFT frontend's frames and spectrum, the LayerNorm rows a stage's last
block hands the downsample, the arrays of the two-GEMM MLPs, the fp32 downsample's xnorm, the segment embeddings, the scene rows of
the class-tiled head).  The driver refuses a plan in which a tenant does not fit (ACX_ERR_STATE before the first launch); this file
shows that no shape a caller can ask for is refused, and that what the promise of acx_workspace_bytes* covers is what the plans use:

  * regions: 256-byte aligned, pairwise disjoint, inside their sub-batch;
  * sub-batches: disjoint, first byte 0, last byte <= the promise, for every number of ways the library can choose at that batch;
  * tenants: inside their region; two of one phase in one region do not overlap; none shares a byte with a region the same phase
    reads or writes in its own role (the LayerNorm rows against y);
  * every plan lists the tenants its arithmetic, frontend and tail have (counted here, independently), with the sizes restated below.

The hook and the forward call the same functions (forward_tenants, the need_* definitions of acx_internal.h): a definition changed
in one is changed in both.  Plans are filled a chunk at a time and checked as numpy arrays over the chunk.
"""
import ctypes
import functools
import random

import numpy as np
import pytest

from audioset_convnext_inf_amd import _ffi

HOP, MIN_L = 320, _ffi.MIN_SAMPLES
DIMS, DEPTHS, STEM_W, MELS, DENSE_N, NFFT = (96, 192, 384, 768), (3, 3, 9, 3), 56, 224, 1056, 1024
PRECS = ("fp32", "bf16", "fp32_split", "bf16a")
TAILS = ("logits", "scene", "frame", "segment", "segment_embeddings")
CLASSES = (1, 527, 4096, 32768)
HEAD_TILED_MIN = 640
# T = 24 (the shortest clip) through two periods of the stage heights (H3 = ((T + 4) / 4 + 1) / 8 repeats every 32 frames): L in steps
# of one hop, one sample either side of each step; then 10 s and 30 s
SWEEP_L = sorted({L for k in range(65) for L in (MIN_L + k * HOP - 1, MIN_L + k * HOP, MIN_L + k * HOP + 1) if L >= MIN_L}
                 | {320000, 960000})
SWEEP_B = tuple(range(1, 41)) + (64, 256)
R = {n: i for i, n in enumerate(_ffi.PLAN_REGIONS)}
K = {n: i for i, n in enumerate(_ffi.PLAN_TENANTS)}
CHUNK = 1024
BIG = 1 << 62


def ways_for(B):
    """every number of sub-batches the library can run B clips as (ACX_SPLIT_WAYS 1 .. 4, eight clips per sub-batch)"""
    return [w for w in (1, 2, 3, 4) if w == 1 or B >= 8 * w]


def describe(what):
    prec, dense, driver, tail, B, L, lengths, classes, head_path, ways, wave, lam = what
    shape = "L=%d" % L if lengths is None else "lengths=%s" % (lengths if len(lengths) <= 6 else lengths[:6] + ["..."],)
    return "%s %s %s %s B=%d %s N=%d head_path=%d ways=%d wave=%d lam=%d" % (prec, "dense" if dense else "auto", driver, tail, B, shape,
                                                                            classes, head_path, ways, wave, lam)


@functools.lru_cache(maxsize=None)
def expected_tenants(prec, dense, driver, tail, tiled):
    """How many tenants one sub-batch's plan must list (the augmented driver's own two not counted)."""
    n = {"fp32": 3 + 2 * (DEPTHS[2] + DEPTHS[3]), "fp32_split": 3 + 3 + DEPTHS[3], "bf16": 3 + 3 + 2 * DEPTHS[3],
         "bf16a": 3 + 3 + 2 * DEPTHS[3]}[prec]
    if dense and driver in ("uniform", "windows", "varlen"):
        n += 2
    if tail == "segment" or (tail == "logits" and tiled):
        n += 1
    return n


class _Bucket:
    def __init__(self):
        self.plans = (_ffi.AcxForwardPlan * CHUNK)()
        self.view = np.frombuffer(self.plans, dtype=np.dtype(_ffi.AcxForwardPlan))
        self.refs = [ctypes.byref(self.plans[i]) for i in range(CHUNK)]
        self.params, self.expect = [], []


class Sweep:
    """Fills plans a chunk at a time and checks each chunk as arrays; keeps the count and the tightest tenant of each kind.  Plans
    of one arithmetic and one number of ways share a chunk: its arrays then hold live sub-batches and tenants only."""

    def __init__(self):
        self.buckets = {}
        self.q = _ffi.AcxForwardPlanQuery()
        self.qref = ctypes.byref(self.q)
        self.fn = _ffi.lib().acx_test_forward_plan
        self.count = 0
        self.bad = []
        self.tight = {}                 # kind -> (used / capacity, used, capacity, params)
        self._keep = None

    def add(self, prec, driver, tail, B, L=MIN_L, lengths=None, dense=False, classes=527, head_path=0, ways=1, wave=False, lam=False):
        q = self.q
        q.precision, q.dense, q.classes, q.head_path = _ffi.PRECISIONS[prec], int(dense), classes, head_path
        q.driver, q.tail, q.ways, q.B = _ffi.PLAN_DRIVERS[driver], _ffi.PLAN_TAILS[tail], ways, B
        q.has_wave_plan, q.has_lambda, q.L = int(wave), int(lam), L
        if lengths is not None:
            self._keep = (ctypes.c_int64 * len(lengths))(*lengths)
            q.lengths = ctypes.cast(self._keep, ctypes.POINTER(ctypes.c_int64))
        bk = self.buckets.get((prec, ways))
        if bk is None:
            bk = self.buckets[(prec, ways)] = _Bucket()
        rc = self.fn(self.qref, bk.refs[len(bk.params)])
        what = (prec, dense, driver, tail, B, L, lengths, classes, head_path, ways, wave, lam)
        assert rc == 0, (describe(what), _ffi.lib().acx_last_error())
        tiled = head_path == 2 or (head_path == 0 and classes >= HEAD_TILED_MIN)
        bk.params.append(what)
        bk.expect.append((expected_tenants(prec, dense, driver, tail, tiled), 2 if driver == "augmented" and dense else 0, ways))
        if len(bk.params) == CHUNK:
            self.flush(bk)

    def flush(self, bk):
        n = len(bk.params)
        if n:
            self.bad += violations(bk.view[:n], bk.params, bk.expect, self.tight)
            self.count += n
        bk.params, bk.expect = [], []

    def report(self, title):
        for bk in self.buckets.values():
            self.flush(bk)
        print("\n%s: %d plans" % (title, self.count))
        for kind in sorted(self.tight):
            ratio, used, cap, what = self.tight[kind]
            print("  tightest %-16s %12d / %12d bytes (%.4f)  %s" % (_ffi.PLAN_TENANTS[kind], used, cap, ratio, describe(what)))
        assert not self.bad, "\n".join(self.bad[:20])


def violations(arr, params, expect, tight):
    """Every way the plans of arr (a structured array over acx_forward_plan_t) break the contract, as strings."""
    out = []

    def report(mask, what):
        for idx in np.argwhere(mask)[:3]:
            out.append("%s: %s at %s" % (what, describe(params[idx[0]]), tuple(int(i) for i in idx[1:])))

    i64 = lambda a: a.astype(np.int64)
    ns, total, promised = i64(arr["n_subs"]), i64(arr["total"]), i64(arr["promised"])
    W = int(min(max(int(ns.max()), 1), _ffi.PLAN_MAX_WAYS))          # (arrays over the live sub-batches and tenants only)
    subs = arr["subs"][:, :W]
    live_sub = np.arange(W)[None, :] < ns[:, None]
    report((ns > W)[:, None], "more sub-batches than the plan holds")
    base, sbytes = i64(subs["base"]), i64(subs["bytes"])
    roff, rby = i64(subs["regions"]["offset"]), i64(subs["regions"]["bytes"])
    live_r = (rby > 0) & live_sub[:, :, None]
    exp_n, exp_aug, exp_ways = (np.array(c) for c in zip(*expect))
    report((ns != exp_ways)[:, None], "number of sub-batches")

    # regions: aligned, inside the sub-batch, pairwise disjoint; the core regions all exist
    report(live_r & ((roff % 256 != 0) | (rby % 256 != 0)), "region not 256-byte aligned")
    report(live_r & ((roff < base[:, :, None]) | (roff + rby > (base + sbytes)[:, :, None])), "region outside its sub-batch")
    report(live_sub[:, :, None] & ~live_r[:, :, R["feat"]:R["stats"] + 1], "region missing")
    o = np.where(live_r, roff, BIG)
    order = np.argsort(o, axis=2, kind="stable")
    so = np.take_along_axis(o, order, 2)
    se = so + np.take_along_axis(np.where(live_r, rby, 0), order, 2)
    report((so[:, :, 1:] < BIG) & (se[:, :, :-1] > so[:, :, 1:]), "regions overlap")

    # sub-batches: from byte 0 on, disjoint, all of them inside the promise
    report((base[:, 0] != 0)[:, None], "first sub-batch does not start at byte 0")
    report(live_sub[:, 1:] & (base[:, :-1] + sbytes[:, :-1] > base[:, 1:]), "sub-batches overlap")
    end = np.where(live_sub, base + sbytes, 0).max(axis=1)
    report(((end != total) | (total > promised))[:, None], "plans end past the promised bytes")
    report((np.where(live_sub, subs["clips"], 0).sum(axis=1) <= 0)[:, None], "no clips")

    # tenants
    nt = i64(subs["n_tenants"])
    report(nt > _ffi.PLAN_MAX_TENANTS, "more tenants than the plan holds")
    TM = int(min(max(int(nt.max()), 1), _ffi.PLAN_MAX_TENANTS))
    t = subs["tenants"][:, :, :TM]
    live_t = (np.arange(TM)[None, None, :] < nt[:, :, None]) & live_sub[:, :, None]
    want = np.where(live_sub, exp_n[:, None], 0)
    want[:, 0] += exp_aug
    report(nt * live_sub != want, "number of tenants")
    kind, region, phase, stage, block = (i64(t[k]) for k in ("kind", "region", "phase", "stage", "block"))
    toff, tby, ops = i64(t["offset"]), i64(t["bytes"]), i64(t["operands"])
    region = np.clip(region, 0, len(R) - 1)
    cap = np.take_along_axis(rby, region, 2)
    start = np.take_along_axis(roff, region, 2) + toff
    report(live_t & ((tby <= 0) | (toff < 0) | (toff + tby > cap)), "tenant outside its region")
    # two tenants of one phase in one region
    key = ((phase * 8 + stage + 1) * 16 + block + 1) * 16 + region
    comp = np.where(live_t, (key << 45) | start, BIG)
    order = np.argsort(comp, axis=2, kind="stable")
    sc = np.take_along_axis(comp, order, 2)
    sstart = np.take_along_axis(start, order, 2)
    send = sstart + np.take_along_axis(tby, order, 2)
    report((sc[:, :, 1:] < BIG) & ((sc[:, :, 1:] >> 45) == (sc[:, :, :-1] >> 45)) & (send[:, :, :-1] > sstart[:, :, 1:]),
           "tenants of one phase overlap")
    # the operand sets, restated here (not taken from the plan): what each phase reads or writes in its own role, from the launch
    # order of run_forward -- the frontend and stem write feat (acx_forward_augmented's own frontend: its wave and feat regions), block
    # j of stage s reads x[s] and y, the downsample in front of stage s reads x[s - 1] and writes x[s], the tail reads x[3]; every
    # phase of a window or variable-length batch reads the tables
    tab, x0 = 1 << R["tables"], R["x0"]
    sclip = np.clip(stage, 0, 3)
    in_aug = region >= R["aug_wave"]
    want_ops = np.select(
        [phase == 0, phase == 1, phase == 2, phase == 3],
        [np.where(in_aug, (1 << R["aug_wave"]) | (1 << R["aug_feat"]), tab | (1 << R["feat"])),
         tab | (1 << (x0 + sclip)) | (1 << R["y"]),
         tab | (1 << (x0 + np.clip(sclip - 1, 0, 3))) | (1 << (x0 + sclip)),
         np.full_like(stage, tab | (1 << (x0 + 3)))], default=-1)
    report(live_t & (ops != want_ops), "operand regions of a phase")
    report(live_t & (((phase == 1) | (phase == 2)) & ((stage < (phase == 2)) | (stage > 3))), "stage of a phase")
    # a tenant against the regions its phase uses in their own role
    every = int(np.bitwise_or.reduce(np.where(live_t, ops, 0), axis=None))
    for r in range(len(R)):
        if not (every >> r) & 1:
            continue
        used = live_t & (((ops >> r) & 1) == 1) & live_r[:, :, r:r + 1]
        report(used & (start < (roff + rby)[:, :, r:r + 1]) & (start + tby > roff[:, :, r:r + 1]),
               "tenant shares bytes with operand region %s" % _ffi.PLAN_REGIONS[r])
    # the tightest tenant of each kind
    ratio = np.where(live_t & (cap > 0), (toff + tby) / np.maximum(cap, 1), 0.0)
    for k in range(len(K)):
        rk = np.where(kind == k, ratio, 0.0)
        if not rk.any():
            continue
        at = np.unravel_index(int(np.argmax(rk)), rk.shape)
        if rk[at] > tight.get(k, (0.0,))[0]:
            tight[k] = (float(rk[at]), int((toff + tby)[at]), int(cap[at]), params[at[0]])
    return out


def tails_and_heads():
    """(tail, classes, head_path): every tail; the class counts on both head paths where a head runs."""
    for tail in TAILS:
        if tail in ("logits", "segment"):
            for n in CLASSES:
                for path in (1, 2):
                    yield tail, n, path
        else:
            yield tail, 527, 0


def test_uniform_and_window_plans_over_every_shape():
    sw = Sweep()
    heads = list(tails_and_heads())
    for L in SWEEP_L:
        for B in SWEEP_B:
            for ways in ways_for(B):
                for prec in PRECS:
                    for dense in (False, True):
                        for tail, n, path in heads:
                            sw.add(prec, "uniform", tail, B, L, dense=dense, classes=n, head_path=path, ways=ways)
                        # the windows driver: the same sub-batches behind the window table
                        sw.add(prec, "windows", "logits", B, L, dense=dense, classes=4096, ways=ways)
                        sw.add(prec, "windows", "segment", B, L, dense=dense, ways=ways)
    sw.report("uniform / windows")


def test_features_and_augmented_plans_over_every_shape():
    sw = Sweep()
    for L in SWEEP_L:
        for B in SWEEP_B:
            for prec in PRECS:
                for tail, n in (("logits", 527), ("logits", 4096), ("scene", 527), ("frame", 527)):
                    for ways in ways_for(B):
                        sw.add(prec, "features", tail, B, L, classes=n, ways=ways)
                    for dense in (False, True):
                        for wave in (False, True):
                            for lam in (False, True):
                                if lam and B % 2:
                                    continue
                                for ways in ways_for(B // 2 if lam else B):
                                    sw.add(prec, "augmented", tail, B, L, dense=dense, classes=n, ways=ways, wave=wave, lam=lam)
    sw.report("features / augmented")


def varlen_batches():
    rng = random.Random(20251)
    edge = (7360, 7361, 7679, 7680, 16000, 17000, 23000, 10239, 10240, 320000)
    out = [[MIN_L] * n for n in (1, 2, 3, 7, 64, 255, 256)]                       # all-minimum lengths
    out += [[MIN_L] * a + [big] + [MIN_L] * b for a, b in ((0, 1), (1, 0), (3, 3), (0, 255), (255, 0), (100, 155))
            for big in (960000, 320001)]                                           # one long clip among minimum ones
    for n in list(range(1, 41)) + [64, 100, 128, 200, 255, 256]:
        for _ in range(3):
            out.append([rng.choice(edge) if rng.random() < 0.3 else rng.randrange(MIN_L, 7360 + 64 * HOP) for _ in range(n)])
        out.append([rng.randrange(MIN_L, 960001) for _ in range(n)])
    return out


def test_varlen_plans():
    sw = Sweep()
    for lengths in varlen_batches():
        for prec in PRECS:
            for dense in (False, True):
                for tail, n, path in tails_and_heads():
                    sw.add(prec, "varlen", tail, len(lengths), lengths=lengths, dense=dense, classes=n, head_path=path)
    sw.report("varlen")


def stage_rows(L):
    T = L // HOP + 1
    h = [(T + 4) // 4 + 1]
    for _ in range(3):
        h.append(h[-1] // 2)
    return T, h


@pytest.mark.parametrize("prec", PRECS)
def test_tenant_sizes_restated(prec):
    """The bytes of every tenant of a few plans, restated from the layouts the launchers document: fp32 rows of C, S16 rows of two
    fp16 halves per element, bf16 rows padded to 64 channels, [M][4C] hidden activations, 1024 + 1056 floats per dense frame."""
    pad64 = lambda c: (c + 63) // 64 * 64
    for B, L in ((1, 7360), (3, 17000), (17, 23000), (5, 320000)):
        T, H = stage_rows(L)
        M = [B * H[s] * (STEM_W >> s) for s in range(4)]
        for tail, n in (("logits", 4096), ("segment", 527)):
            p = _ffi.forward_plan(prec, "uniform", tail, B, L, dense=True, classes=n)
            sub = p.subs[0]
            assert sub.regions[R["y"]].bytes >= M[0] * 96 * 4 and sub.regions[R["hidden"]].bytes >= M[0] * 384 * 4
            assert sub.regions[R["feat"]].bytes >= B * T * MELS * 4 and sub.regions[R["stats"]].bytes >= M[0] * 8
            for i in range(sub.n_tenants):
                t = sub.tenants[i]
                name, s = _ffi.PLAN_TENANTS[t.kind], t.stage
                want = {"dense_frames": lambda: B * T * NFFT * 4, "dense_spec": lambda: B * T * DENSE_N * 4,
                        "ln_rows": lambda: (M[s] if t.phase == 1 else M[s - 1]) * (DIMS[s if t.phase == 1 else s - 1] * 4 if prec == "fp32_split"
                                                                                   else pad64(DIMS[s if t.phase == 1 else s - 1]) * 2),
                        "mlp_bf16_hidden": lambda: M[s] * 4 * DIMS[s] * 2, "mlp_bf16_rows": lambda: M[s] * pad64(DIMS[s]) * 2,
                        "hidden_act": lambda: M[s] * 4 * DIMS[s] * 4, "row_stats": lambda: M[s] * 8,
                        "xnorm": lambda: M[s - 1] * DIMS[s - 1] * 4, "segment_emb": lambda: B * H[3] * 768 * 4,
                        "scene_rows": lambda: B * 768 * 4}[name]()
                assert t.bytes == want, (name, s, t.block, t.bytes, want)
                assert t.region == {"dense_frames": R["hidden"], "dense_spec": R["y"], "ln_rows": R["hidden"], "mlp_bf16_hidden": R["hidden"],
                                    "mlp_bf16_rows": R["hidden"], "hidden_act": R["hidden"], "row_stats": R["stats"], "xnorm": R["y"],
                                    "segment_emb": R["feat"], "scene_rows": R["feat"]}[name]


def test_promise_equals_the_size_calls_and_bad_queries_are_refused():
    lib = _ffi.lib()
    for B, L in ((1, 7360), (17, 16000), (33, 7360), (64, 23000)):
        need = ctypes.c_size_t()
        assert lib.acx_workspace_bytes(None, B, L, 0, ctypes.byref(need)) == 0
        assert _ffi.forward_plan("bf16a", "uniform", "logits", B, L).promised == need.value
        assert lib.acx_workspace_bytes_windows(None, B, L, 0, ctypes.byref(need)) == 0
        assert _ffi.forward_plan("bf16a", "windows", "logits", B, L).promised == need.value
    with pytest.raises(_ffi.AcxError):
        _ffi.forward_plan("fp32", "uniform", "logits", 15, 7360, ways=2)            # 8 clips per sub-batch
    with pytest.raises(_ffi.AcxError):
        _ffi.forward_plan("fp32", "varlen", "logits", lengths=[7360, 7359])
    with pytest.raises(_ffi.AcxError):
        _ffi.forward_plan("fp32", "features", "segment", 2, 7360)
    with pytest.raises(_ffi.AcxError):
        _ffi.forward_plan("fp32", "augmented", "logits", 3, 7360, lam=True)
    assert lib.acx_test_forward_plan(None, None) != 0
