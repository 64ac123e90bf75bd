"""Host-side mirror of the reference model surface for the audio-tagging hot path.

Same names, arguments, dict keys, output shapes and state_dict keys as the reference's
`audioset_convnext_inf.pytorch.convnext` (ConvNeXt :130-511, Block :44-87, LayerNorm :514-541,
convnext_tiny :641-708), so demo_convnext.py / evaluate_convnext_on_audioset.py /
pytorch_utils.forward can switch imports and keep working.  Nothing here computes: the modules
below are parameter containers (they give `state_dict()` / `load_state_dict()` /
`safetensors.torch.load_model` the reference's 190 keys) and the three forwards hand raw device
pointers to libacx (HIP kernels, include/acx.h) on the current torch stream.

Inference only, GPU only: there is no CPU fallback and no training branch (the reference's
augmentations / mixup / DropPath only run under `self.training`, convnext.py:288-313).
"""
import ctypes
import os

import torch
import torch.nn as nn

from .. import _ffi
from .. import frontend_tables as ft
from . import resample as _rs
from . import windows as _win
from . import stream as _stream
from . import segments as _seg
from . import sed_metrics as _sed

HF_PYTORCH_WEIGHTS_NAME = "model.safetensors"     # convnext.py:29
HF_CONFIG_NAME = "config.yaml"                    # convnext.py:31

_TINY_DEPTHS = [3, 3, 9, 3]
_TINY_DIMS = [96, 192, 384, 768]


class LayerNorm(nn.Module):
    """Parameter container for the reference LayerNorm (both data formats; convnext.py:514-541)."""

    def __init__(self, normalized_shape, eps=1e-6, data_format="channels_last"):
        super().__init__()
        if data_format not in ("channels_last", "channels_first"):
            raise NotImplementedError
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))
        self.eps = eps
        self.data_format = data_format
        self.normalized_shape = (normalized_shape,)


class Block(nn.Module):
    """Parameter container for one ConvNeXt block (convnext.py:44-87); computed by K3 + K4."""

    def __init__(self, dim, drop_path=0.0, layer_scale_init_value=1e-6):
        super().__init__()
        if drop_path != 0.0:
            raise NotImplementedError("stochastic depth is a training feature; the inference path uses rate 0")
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones((dim)), requires_grad=True)
        self.drop_path = nn.Identity()


class _STFT(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv_real = nn.Conv1d(1, ft.N_BINS, ft.N_FFT, stride=ft.HOP, bias=False)
        self.conv_imag = nn.Conv1d(1, ft.N_BINS, ft.N_FFT, stride=ft.HOP, bias=False)
        real, imag = ft.stft_weights()
        self.conv_real.weight.data = torch.from_numpy(real)
        self.conv_imag.weight.data = torch.from_numpy(imag)
        for p in self.parameters():
            p.requires_grad = False


class Spectrogram(nn.Module):
    """Holds `stft.conv_real.weight` / `stft.conv_imag.weight` like torchlibrosa's module
    (constructed at convnext.py:179-187); evaluated by the FFT inside kernel K1."""

    def __init__(self):
        super().__init__()
        self.stft = _STFT()


class LogmelFilterBank(nn.Module):
    """Holds `melW` (513,224) like torchlibrosa's module (convnext.py:190-200)."""

    def __init__(self):
        super().__init__()
        self.melW = nn.Parameter(torch.from_numpy(ft.mel_matrix()), requires_grad=False)


class ConvNeXt(nn.Module):
    """Drop-in for the reference `ConvNeXt` restricted to what its shipped entry points build:
    ConvNeXt-Tiny, the [252,56] audio stem, 32 kHz / 1024 / 320 / 224-mel frontend.  The classifier head
    (`head_audioset`, convnext.py:257) may have any num_classes N in [1, 32768]: 527 for AudioSet, the task's label count for a
    fine-tuned model; every (B, 527) output below is (B, N) then."""

    def __init__(self, in_chans=3, num_classes=1000, depths=[3, 3, 9, 3], dims=[96, 192, 384, 768],
                 drop_path_rate=0.0, use_pydub_augment=False, use_roll_augment=False, use_speed_perturb=False,
                 use_torchaudio=False, layer_scale_init_value=1e-6, head_init_scale=1.0):
        super().__init__()
        if list(depths) != _TINY_DEPTHS or list(dims) != _TINY_DIMS:
            raise NotImplementedError("the MI355X path implements ConvNeXt-Tiny (convnext_tiny()); "
                                      "got depths=%r dims=%r" % (depths, dims))
        check_num_classes(num_classes)
        if use_torchaudio:
            raise NotImplementedError("use_torchaudio=True (Kaldi fbank input) is outside the inference contract")
        if layer_scale_init_value <= 0:
            raise NotImplementedError("layer scale (gamma) is part of the state_dict contract")
        self.use_torchaudio = False
        self.use_pydub_augment = use_pydub_augment      # training-only switches, kept for signature parity
        self.use_roll_augment = use_roll_augment
        self.use_speed_perturb = use_speed_perturb

        self.spectrogram_extractor = Spectrogram()
        self.logmel_extractor = LogmelFilterBank()
        self.bn0 = nn.BatchNorm2d(224)
        self.downsample_layers = nn.ModuleList()
        self.downsample_layers.append(nn.Sequential(
            nn.Conv2d(1, dims[0], kernel_size=(4, 4), stride=(4, 4), padding=(4, 0)),      # the [252,56] stem
            LayerNorm(dims[0], eps=1e-6, data_format="channels_first")))
        for i in range(3):
            self.downsample_layers.append(nn.Sequential(
                LayerNorm(dims[i], eps=1e-6, data_format="channels_first"),
                nn.Conv2d(dims[i], dims[i + 1], kernel_size=2, stride=2)))
        self.stages = nn.ModuleList()
        for i in range(4):
            self.stages.append(nn.Sequential(*[
                Block(dim=dims[i], drop_path=0.0, layer_scale_init_value=layer_scale_init_value)
                for _ in range(depths[i])]))
        self.norm = nn.LayerNorm(dims[-1], eps=1e-6)
        self.head_audioset = nn.Linear(dims[-1], num_classes)
        self.apply(self._init_weights)
        self.head_audioset.weight.data.mul_(head_init_scale)
        self.head_audioset.bias.data.mul_(head_init_scale)

        self._ctx = {}          # device index -> (_ffi.Context, weight signature)
        # arithmetic of the dense contractions (include/acx.h, enum acx_precision).  "fp32_split" and "fp32" are both
        # fp32-grade (same parity tests, same tolerances); split is the fast one.  ACX_PRECISION overrides the default.
        self.precision = os.environ.get("ACX_PRECISION", "fp32_split")
        self.frontend = os.environ.get("ACX_FRONTEND", "auto")       # set_frontend()
        if self.precision not in _ffi.PRECISIONS:
            raise ValueError("ACX_PRECISION must be one of %s" % sorted(_ffi.PRECISIONS))
        if self.frontend not in _ffi.FRONTENDS:
            raise ValueError("ACX_FRONTEND must be one of %s" % sorted(_ffi.FRONTENDS))
        self._ws = {}           # (device index, stream handle) -> workspace tensor: concurrent forwards on different
        #                         streams never share scratch memory (the reference module is re-entrant in eval).
        #                         Insertion-ordered, most recently used last; at most _WS_MAX_STREAMS entries are kept
        self._ws_captured = set()   # data pointers of workspaces a stream capture has seen: a hipGraph may point into them
        self._ws_retired = []   # replaced workspaces that a captured graph may still reference (only those) stay alive
        self._weights_epoch = 0  # bumped by load_state_dict / _apply / refresh(): forces a repack of the native weights
        self._sig_cache = None  # (epoch, [parameter and buffer tensors]) -- see _signature
        self._resamplers = {}   # (device index, input rate, 32000) -> _ffi.Resampler: the band tables of forward(sample_rate=)

    def _init_weights(self, m):
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            nn.init.trunc_normal_(m.weight, std=0.02)
            nn.init.constant_(m.bias, 0)

    # ------------------------------------------------------------------------------ native side
    def _signature(self):
        """Changes whenever the weights may have: the epoch counter (load_state_dict / _apply / refresh) plus, for every
        parameter and buffer, its identity, storage address and autograd version, plus the identity of every submodule.
        What is cached per epoch is the list of the modules' own `_parameters` / `_buffers` / `_modules` dicts, not the
        tensors: a replaced Parameter (`m.head_audioset.weight = nn.Parameter(...)`) shows up as a new id in its module's
        dict, a replaced submodule (`m.head_audioset = nn.Linear(...)`) as a new child id in its parent's -- the latter
        also rebuilds the cached list.  state_dict() itself builds 190 prefixed keys and cost 0.6 ms per
        forward, ten times the rest of the host path at batch 1 (profiles/r03_f_latency_bs1.txt); this walk costs ~50 us."""
        for _ in range(2):
            c = self._sig_cache
            if c is None or c[0] != self._weights_epoch:
                dicts = [(m._parameters, m._buffers, m._modules) for m in self.modules()]
                c = self._sig_cache = (self._weights_epoch, dicts,
                                       tuple(id(x) for _, _, ch in dicts for x in ch.values()))
            sig = [self.precision, self.frontend, self._weights_epoch]
            kids = []
            for params, bufs, children in c[1]:
                for t in params.values():
                    if t is not None:
                        sig += (id(t), t.data_ptr(), t._version)
                for t in bufs.values():
                    if t is not None:
                        sig += (id(t), t.data_ptr(), t._version)
                kids += [id(x) for x in children.values()]
            if tuple(kids) == c[2]:
                return tuple(sig)
            self._weights_epoch += 1        # the module tree changed: walk it again
        raise RuntimeError("module tree changed while its signature was taken")

    def refresh(self):
        """Call after editing weights in a way autograd's version counters cannot see (`param.data.mul_(...)`, writes
        through numpy views): the native contexts repack the weights at the next forward.  `load_state_dict`, `.to()`,
        `.half()`-style `_apply` calls and ordinary in-place tensor ops are detected without it."""
        self._weights_epoch += 1
        return self

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._weights_epoch += 1
        return out

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._weights_epoch += 1
        # contexts and workspaces of devices the module has left are released
        dev = self.head_audioset.weight.device
        keep = dev.index if dev.type == "cuda" and dev.index is not None else (torch.cuda.current_device() if dev.type == "cuda" else None)
        for idx in [i for i in self._ctx if i != keep]:
            self._ctx.pop(idx)[0].close()
        for key in [k for k in self._ws if k[0] != keep]:
            self._ws.pop(key)
        for key in [k for k in self._resamplers if k[0] != keep]:
            self._resamplers.pop(key).close()
        if keep is None:
            self._ws_retired.clear()
            self._ws_captured.clear()
        return out

    # native handles (ctypes) and scratch tensors are per-process state, rebuilt on demand: field -> its empty value
    _PER_PROCESS = {"_ctx": dict, "_ws": dict, "_resamplers": dict, "_ws_retired": list, "_ws_captured": set,
                    "_sig_cache": lambda: None}

    def __getstate__(self):
        state = self.__dict__.copy()
        state.update((k, make()) for k, make in self._PER_PROCESS.items())
        return state

    def __deepcopy__(self, memo):
        import copy
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = self._PER_PROCESS[k]() if k in self._PER_PROCESS else copy.deepcopy(v, memo)
        return new

    def set_precision(self, precision):
        """"fp32_split" (default): fp32 GEMM operands carried as fp16 hi + fp16 lo, three fp16 MFMAs per product, fp32
        accumulate -- fp32-grade (1e-3 parity), 16/3 of the f32-MFMA rate.  "fp32": v_mfma_f32_32x32x2_f32 on the
        fp32 operands themselves.  "bf16": pointwise / downsample contractions with bf16 operands and fp32
        accumulation (NOT within the 1e-3 bar); LayerNorm, residual stream, depthwise conv, frontend and head stay
        fp32 in every mode.  "bf16a": "bf16" plus the activations of stages 0-2 (residual stream, depthwise-conv output) stored
        in HBM as bf16 -- half the activation bytes; statistics, accumulation, GELU and the residual add stay fp32.
        The reference has no such switch (closest: torch autocast around its nn.Linear layers)."""
        if precision not in _ffi.PRECISIONS:
            raise ValueError("precision must be one of %s" % sorted(_ffi.PRECISIONS))
        self.precision = precision
        return self

    def set_frontend(self, mode):
        """"auto" (default): the FFT kernel evaluates torchlibrosa's STFT whenever the stored `conv_real` / `conv_imag` buffers
        are window x DFT.  "dense": always the reference's own formulation -- the two Conv1d as one dense contraction with the
        stored weights (convnext.py:179-187,298) -- and thereby its rounding: the parity mode for pure tones and clean sweeps,
        whose bins 90 dB under the frame peak the two formulations round differently (include/acx.h, acx_set_frontend)."""
        if mode not in _ffi.FRONTENDS:
            raise ValueError("frontend must be one of %s" % sorted(_ffi.FRONTENDS))
        self.frontend = mode
        return self

    @property
    def num_classes(self):
        """N, the width of the logits and probabilities: the classifier head's out_features (527 for AudioSet)."""
        return self.head_audioset.out_features

    def _check_head(self):
        """A replaced head (`model.head_audioset = nn.Linear(768, N)`) must be a 768 -> N linear map with a bias."""
        h = self.head_audioset
        if not isinstance(h, nn.Linear) or h.in_features != _TINY_DIMS[-1]:
            raise ValueError("head_audioset must be an nn.Linear(768, N) (got %r)" % (h,))
        check_num_classes(h.out_features)
        if h.bias is None:
            raise ValueError("head_audioset.bias is missing: the classifier head needs a bias (nn.Linear(768, %d, bias=True), "
                             "as the reference's head_audioset)" % h.out_features)
        if tuple(h.weight.shape) != (h.out_features, h.in_features) or tuple(h.bias.shape) != (h.out_features,):
            raise ValueError("head_audioset.weight %s / head_audioset.bias %s do not match nn.Linear(768, %d)"
                             % (tuple(h.weight.shape), tuple(h.bias.shape), h.out_features))

    def native_context(self, device):
        """The libacx context holding this module's weights on `device` (rebuilt when they change).  ctx.classes: N."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        sig = self._signature()
        hit = self._ctx.get(idx)
        if hit is not None and hit[1] == sig:
            return hit[0]
        self._check_head()
        ctx = hit[0] if hit is not None else _ffi.Context(idx)
        ctx.set_precision(self.precision)
        ctx.set_frontend(self.frontend)
        ctx.load_state_dict(self.state_dict())
        ctx.classes = ctx.num_classes()
        self._ctx[idx] = (ctx, sig)
        return ctx

    _WS_MAX_STREAMS = 8      # workspaces kept per module (one per (device, stream) in use); the least recently used goes first

    def _workspace(self, device, nbytes):
        """Scratch memory of one forward on (device, current stream).  Grows geometrically (a length-sorted sweep would
        otherwise reallocate at every new maximum); a replaced or evicted workspace is freed unless a stream capture has
        seen it -- a captured hipGraph replays with the pointers it recorded, so those stay alive with the module."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        key = (idx, torch.cuda.current_stream(device).cuda_stream)
        ws = self._ws.pop(key, None)
        if ws is None or ws.numel() < nbytes:
            if ws is not None:
                self._retire(ws)
                nbytes = max(nbytes, ws.numel() + ws.numel() // 2)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self._ws[key] = ws                      # (re-)inserted last: most recently used
        while len(self._ws) > self._WS_MAX_STREAMS:
            self._retire(self._ws.pop(next(iter(self._ws))))
        if torch.cuda.is_current_stream_capturing():
            self._ws_captured.add(ws.data_ptr())
        return ws

    def _retire(self, ws):
        if ws.data_ptr() in self._ws_captured:
            self._ws_retired.append(ws)

    @staticmethod
    def _check_batch(x):
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise ValueError("expected a (batch, samples) waveform tensor, got %r" % (getattr(x, "shape", type(x)),))

    def _check_run(self, device):
        if self.training:
            raise RuntimeError("inference-only path: call model.eval() first (the reference's training branches -- "
                               "augmentations, SpecAugment, mixup -- are not part of this build)")
        wdev = self.head_audioset.weight.device
        if wdev.type != "cuda" or device.type != "cuda":
            raise RuntimeError("the MI355X path runs on the GPU only (model on %s, input on %s): "
                               "move both with .to('cuda'); there is no CPU fallback" % (wdev, device))
        if device != wdev:
            raise RuntimeError("input on %s but model on %s" % (device, wdev))

    @staticmethod
    def _outputs(kind, lead, classes, L, device, clips=None):
        """The (out0, out1, clip) of one ABI call of output kind `kind` (a key of _ffi.MODES or _ffi.SEG_WHAT).  `lead`: the
        leading shape -- clips or windows of L samples each, or (L = None) the packed rows of a variable-length batch, whose
        "segment" clip maxima have `clips` rows.  What a kind does not have is None."""
        def new(*shape):
            return torch.empty(shape, dtype=torch.float32, device=device)
        if kind == "logits":
            return new(*lead, classes), new(*lead, classes), None
        if kind == "scene":
            return new(*lead, 768), None, None
        if kind == "frame":
            return (new(*lead) if L is None else new(*lead, 768, *_ffi.stage_hw(L, 3))), None, None
        if L is not None:
            lead = lead + (_seg.segment_count(L),)
        if kind == "segment":
            return new(*lead, classes), new(*lead, classes), new(lead[0] if clips is None else clips, classes)
        return new(*lead, 768), None, None

    # The three runners: one ABI call (windows: one per max_batch windows) of any output kind on packed 32 kHz fp32 audio.  Each
    # returns (out0, out1, clip) as _outputs names them; `pool` matters to the two segment kinds only.
    def _run(self, x, kind, pool=3):
        """(B, L) -> acx_forward / acx_forward_segments."""
        self._check_batch(x)
        self._check_run(x.device)
        x = x.detach().to(torch.float32).contiguous()
        B, L = x.shape
        if L < _ffi.MIN_SAMPLES:
            raise RuntimeError("clip of %d samples is too short: kernel size can't be greater than actual input size "
                               "(minimum is %d samples)" % (L, _ffi.MIN_SAMPLES))
        dev, seg = x.device, _ffi.SEG_WHAT.get(kind)
        with torch.cuda.device(dev):
            ctx = self.native_context(dev)
            ws = self._workspace(dev, ctx.workspace_bytes(B, L, kind))
            out0, out1, clip = self._outputs(kind, (B,), ctx.classes, L, dev)
            if seg is None:
                _ffi.check(_ffi.lib().acx_forward(ctx.handle, _ffi.ptr(x), B, L, _ffi.MODES[kind], _ffi.ptr(out0), _ffi.ptr(out1),
                                                  _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr(dev)))
            else:
                _ffi.check(_ffi.lib().acx_forward_segments(ctx.handle, _ffi.ptr(x), B, L, pool, seg, _ffi.ptr(out0), _ffi.ptr(out1),
                                                           _ffi.ptr(clip), _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr(dev)))
        return out0, out1, clip

    def _run_varlen(self, wav, lengths, kind, pool=3):
        """wav: packed 1-D tensor, lengths: list of <= 256 ints summing to wav.numel() -> acx_forward_varlen /
        acx_forward_segments_varlen.  Frame blocks (varlen_frame_layout) and segment rows (sum(S_i)) lie back to back."""
        B, dev, seg = len(lengths), wav.device, _ffi.SEG_WHAT.get(kind)
        if kind == "frame":
            lead = (varlen_frame_layout(lengths)[-1],)
        else:
            lead = (B if seg is None else sum(_seg.segment_count(n) for n in lengths),)
        with torch.cuda.device(dev):
            ctx = self.native_context(dev)
            ws = self._workspace(dev, ctx.workspace_bytes_varlen(lengths, kind))
            out0, out1, clip = self._outputs(kind, lead, ctx.classes, None, dev, clips=B)
            lens = (ctypes.c_int64 * B)(*lengths)
            if seg is None:
                _ffi.check(_ffi.lib().acx_forward_varlen(ctx.handle, _ffi.ptr(wav), lens, B, _ffi.MODES[kind], _ffi.ptr(out0),
                                                         _ffi.ptr(out1), _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr(dev)))
            else:
                _ffi.check(_ffi.lib().acx_forward_segments_varlen(ctx.handle, _ffi.ptr(wav), lens, B, pool, seg, _ffi.ptr(out0),
                                                                  _ffi.ptr(out1), _ffi.ptr(clip), _ffi.ptr(ws), ws.numel(),
                                                                  _ffi.stream_ptr(dev)))
        return out0, out1, clip

    def _run_windows(self, wav, lengths, W, H, kind, max_batch, pool=3):
        """Every window of recordings longer than W (<= 256, packed in wav) -> acx_forward_windows /
        acx_forward_segments_windows, max_batch at a time: one row (frame, segment kinds: one block) per window, in window
        order."""
        n = _ffi.window_count(lengths, W, H)
        dev, seg = wav.device, _ffi.SEG_WHAT.get(kind)
        with torch.cuda.device(dev):
            ctx = self.native_context(dev)
            out0, out1, clip = self._outputs(kind, (n,), ctx.classes, W, dev)
            ws = self._workspace(dev, ctx.workspace_bytes_windows(min(n, max_batch), W, kind))
            lens = (ctypes.c_int64 * len(lengths))(*lengths)
            for first in range(0, n, max_batch):
                count = min(max_batch, n - first)
                o0, o1, cl = (None if t is None else _ffi.ptr(t[first:first + count]) for t in (out0, out1, clip))
                if seg is None:
                    _ffi.check(_ffi.lib().acx_forward_windows(ctx.handle, _ffi.ptr(wav), lens, len(lengths), W, H, first, count,
                                                              _ffi.MODES[kind], o0, o1, _ffi.ptr(ws), ws.numel(),
                                                              _ffi.stream_ptr(dev)))
                else:
                    _ffi.check(_ffi.lib().acx_forward_segments_windows(ctx.handle, _ffi.ptr(wav), lens, len(lengths), W, H, first,
                                                                       count, pool, seg, o0, o1, cl, _ffi.ptr(ws), ws.numel(),
                                                                       _ffi.stream_ptr(dev)))
        return out0, out1, clip

    def _rate(self, sample_rate):
        """None when the input is at the model rate (today's path, nothing extra launched), else the checked integer rate."""
        if sample_rate is None:
            return None
        rate = _rs.check_rate(sample_rate)
        return None if rate == _rs.MODEL_RATE else rate

    def _resampled(self, x, sample_rate):
        """(B, L) at sample_rate -> (B, ceil(nf L / of)) at 32 kHz, on x's stream (acx_resample)."""
        rate = self._rate(sample_rate)
        if rate is None:
            return x
        self._check_batch(x)
        self._check_run(x.device)
        _rs.check_min_length(x.shape[1], rate)
        return _rs.resample(x, rate, _rs.MODEL_RATE, _cache=self._resamplers)

    def _check_segment_call(self, pool):
        """ValueError for a bad pool or a model in train mode, before anything touches the GPU."""
        _seg.check_pool(pool)
        if self.training:
            raise ValueError("inference-only path: call model.eval() first (segment outputs have no training branch)")

    def forward_segments(self, x, pool=3, resolution="segment", sample_rate=None):
        """Sound event detection: WHEN inside a clip something happens, at the cost of one forward.  The reference's
        decision-level recipe (pytorch/models.py:5757-5771) on this trunk's stage-3 map, whose rows are segments of 0.32 s
        (pytorch/segments.py): mean over frequency, max + average over `pool` segments (odd, 1 .. 31), the final LayerNorm and
        the head per segment, sigmoid.  (B, L) -> dict:
          "segmentwise_logits" / "segmentwise_output"  (B, S, N), S = L // 10240 up to rounding (segments.segment_count);
          "clipwise_output"   (B, N), the maximum over segments (models.py:5767) -- NOT model(x)["clipwise_output"], which
                              pools the whole clip before the head;
          "segment_edges"     float64 CPU tensor of S + 1 boundaries in seconds of the input audio;
          "framewise_output"  (B, T, N) with resolution="frame": every segment repeated over its 32 STFT frames, the last one to
                              the clip's end (interpolate + pad_framewise_output, pytorch_utils.py:140-176) -- the key
                              pytorch/inference.py:156 (sound_event_detection) reads.
        The tail is fp32 in every precision mode.  A clip's rows are bit-identical alone, anywhere in a batch, through
        forward_varlen and as a window of forward_windows.  The reference ConvNeXt was trained with global pooling only: these
        are its decision-level recipe applied to it, not outputs its authors evaluated."""
        self._check_segment_call(pool)
        if resolution not in ("segment", "frame"):
            raise ValueError("resolution must be 'segment' or 'frame' (got %r)" % (resolution,))
        rate = self._rate(sample_rate)
        x_in = x
        x = self._resampled(x_in, sample_rate)
        logits, probs, clip = self._run(x, "segment", pool)
        B, S, N = probs.shape
        L = x.shape[1]
        duration = None if rate is None else x_in.shape[1] / rate        # (both calls above have checked the input's shape)
        out = {"segmentwise_logits": logits, "segmentwise_output": probs, "clipwise_output": clip,
               "segment_edges": torch.from_numpy(_seg.segment_edges(L, duration))}
        if resolution == "frame":
            T = _ffi.num_frames(L)
            frame = torch.empty((B, T, N), dtype=torch.float32, device=x.device)
            with torch.cuda.device(x.device):
                _ffi.check(_ffi.lib().acx_segment_expand(_ffi.ptr(probs), B, S, N, T, _ffi.ptr(frame), _ffi.stream_ptr(x.device)))
            out["framewise_output"] = frame
        return out

    def detect_events(self, waveform, pool=3, sample_rate=None, **decode_args):
        """forward_segments followed by the event decoding, both on the GPU and on the same stream: WHAT happens WHEN, as a
        table.  Returns forward_segments' dict (segment resolution) plus "events": an EventTable over the batch, decoded from
        "segmentwise_output" with the clip's "segment_edges" (pytorch/segments.py, decode_events_gpu).  decode_args: threshold,
        low, median, min_duration, merge_gap, capacity -- decode_events' arguments; they are checked before the forward runs.
        threshold / low may hold one value per class (an array, or a CUDA tensor such as metrics.operating_points(...).threshold,
        whose values are checked on the device when the table is first read).
        Nothing synchronises until the table is read (len(), .to_lists(labels), .check())."""
        if "step" in decode_args or "steps" in decode_args:
            raise TypeError("detect_events takes its boundaries from the clip: step / steps are not arguments")
        _seg.check_event_args(decode_args.get("threshold", 0.5), decode_args.get("low"), decode_args.get("median", 1),
                              decode_args.get("min_duration", 0.0), decode_args.get("merge_gap", 0.0), classes=self.num_classes)
        out = self.forward_segments(waveform, pool=pool, sample_rate=sample_rate)
        out["events"] = _seg.decode_events_gpu(out["segmentwise_output"], step=out["segment_edges"].numpy(), **decode_args)
        return out

    def score_events(self, waveform, reference, metric="event", **args):
        """detect_events followed by the scoring of its table against annotated events, all on the GPU and on the same stream
        (pytorch/sed_metrics.py).  reference: a ReferenceEvents on the model's device, one entry per clip of the batch;
        metric: "event" (onset / offset collars), "segment" (a fixed time grid) or "intersection" (the criteria of PSDS).
        args: detect_events' own (pool, sample_rate, threshold, low, median, min_duration, merge_gap, capacity) and the
        scorer's (t_collar, percentage_of_length, evaluate_onset, evaluate_offset / time_resolution / dtc_threshold,
        gtc_threshold, cttc_threshold).  Returns detect_events' dict plus "scores",
        a SedScores; nothing synchronises until the table or the scores are read."""
        args = dict(args)
        score, score_args = _sed._scorer(metric, args)
        out = self.detect_events(waveform, **args)
        out["scores"] = score(reference, out["events"], **score_args)
        return out

    def psds(self, waveform, reference, pool=3, sample_rate=None, **psds_args):
        """forward_segments followed by sed_metrics.psds on "segmentwise_output" with the clips' own "segment_edges": the
        polyphonic sound detection score of the batch against a ReferenceEvents on the model's device, one forward and a
        sweep of thresholds decoded and scored on the GPU.  psds_args: thresholds, scenario ("dcase_1" / "dcase_2"),
        dtc_threshold, gtc_threshold, cttc_threshold, alpha_ct, alpha_st, max_efpr, unit_seconds and the decoder's (low, median,
        min_duration, merge_gap, capacity); psds' own are checked before the forward runs.  Returns forward_segments' dict
        plus "psds", a sed_metrics.PsdsResult."""
        if "step" in psds_args or "steps" in psds_args:
            raise TypeError("psds takes its boundaries from the clip: step / steps are not arguments")
        if "threshold" in psds_args:
            raise TypeError("psds sets threshold itself")
        own = ("thresholds", "scenario", "dtc_threshold", "gtc_threshold", "cttc_threshold", "alpha_ct", "alpha_st", "max_efpr",
               "unit_seconds")
        _sed.check_psds_args(**{k: psds_args[k] for k in own if k in psds_args})
        out = self.forward_segments(waveform, pool=pool, sample_rate=sample_rate)
        out["psds"] = _sed.psds(out["segmentwise_output"], reference, step=out["segment_edges"].numpy(), **psds_args)
        return out

    def tag(self, waveform, threshold, sample_rate=None, calibration=None):
        """Tags as decisions: one forward, then clipwise_output >= threshold.  threshold: one number, or one per class (an
        array, or a CUDA tensor such as metrics.operating_points(...).threshold; +inf: the class never fires).  calibration: a
        calibration.PlattScaling -- its probabilities of the logits take the place of clipwise_output, in the comparison and in
        the result.  Returns {"labels": bool (B, N), "clipwise_output", "clipwise_logits"}; nothing synchronises."""
        if isinstance(threshold, torch.Tensor):
            thr = threshold.detach()
        else:
            thr = torch.as_tensor(threshold, dtype=torch.float32)
        N = self.num_classes
        if thr.dim() > 1 or (thr.dim() == 1 and thr.shape[0] != N):
            raise ValueError("threshold of shape %r for %d classes (expected a number or (%d,))" % (tuple(thr.shape), N, N))
        if not thr.is_cuda and bool(torch.isnan(thr).any()):
            raise ValueError("threshold holds a NaN")
        out = self(waveform, sample_rate=sample_rate)
        probs = out["clipwise_output"]
        if calibration is not None:
            from . import calibration as _cal
            if not isinstance(calibration, _cal.PlattScaling):
                raise ValueError("tag(calibration=) takes a PlattScaling (got %s)" % type(calibration).__name__)
            probs = calibration.apply(out["clipwise_logits"])
        return {"labels": probs >= thr.to(device=probs.device, dtype=probs.dtype), "clipwise_output": probs,
                "clipwise_logits": out["clipwise_logits"]}

    def classify(self, waveform, k=5, sample_rate=None, calibration=None):
        """A single-label head (fit_head(..., loss="ce")) read with softmax: one forward, then classify.softmax_topk on the same
        stream; nothing synchronises.  calibration: a calibration.TemperatureScaling -- the softmax is taken of its scaled
        logits; clipwise_logits stay raw.  Returns {"probabilities" (B, N), "labels" (B,) int64 = the top-1 class, "top_indices"
        (B, k) int32, "top_probabilities" (B, k), "clipwise_logits"}; k is cut to N.  model(x) itself keeps returning the sigmoid
        clipwise_output ("Single-label heads")."""
        from . import classify as _cl
        logits = self(waveform, sample_rate=sample_rate)["clipwise_logits"]
        scaled = logits
        if calibration is not None:
            from . import calibration as _cal
            if not isinstance(calibration, _cal.TemperatureScaling):
                raise ValueError("classify(calibration=) takes a TemperatureScaling (got %s)" % type(calibration).__name__)
            scaled = calibration.apply(logits)
        probs, top_prob, top_index = _cl.softmax_topk(scaled, k=min(int(k), int(logits.shape[1])))
        return {"probabilities": probs, "labels": top_index[:, 0].to(torch.int64), "top_indices": top_index,
                "top_probabilities": top_prob, "clipwise_logits": logits}

    def forward_segment_embeddings(self, x, pool=3, sample_rate=None):
        """(B, L) -> (B, S, 768): the embedding of every 0.32 s segment -- forward_segments' rows in front of the head, i.e.
        forward_scene_embeddings' recipe (convnext.py:279-285) with the pooling over `pool` segments instead of the clip.  The
        rows are valid fit_head / tagging_metrics inputs as they are (`.reshape(-1, 768)`), so a head can be trained and scored
        on strong labels."""
        self._check_segment_call(pool)
        return self._run(self._resampled(x, sample_rate), "segment_embeddings", pool)[0]

    def forward_varlen(self, clips, lengths=None, what="logits", sample_rate=None, pool=3):
        """Clips of different lengths in one packed forward (acx_forward_varlen); every clip's result is bit-identical to the
        uniform forward of that clip alone.  clips: a list of 1-D CUDA tensors, or one packed 1-D CUDA tensor plus `lengths`.
        what: "logits" -> {"clipwise_output", "clipwise_logits"} each (B, N); "scene" -> (B, 768); "frame" -> a list of
        (768, T'_i, 7) views into one output buffer; "segment" -> a list with one dict per clip, "segmentwise_logits" /
        "segmentwise_output" (S_i, N) and "clipwise_output" (N,), the maximum over the clip's segments; "segment_embeddings" ->
        a list of (S_i, 768) views (forward_segments / forward_segment_embeddings with `pool`).  More than 256 clips run as
        several calls.
        sample_rate: the clips' rate (lengths count input samples); other than None / 32000 they are resampled to 32 kHz on
        the device first (acx_resample), each clip's bits the same as model(clip[None], sample_rate=...)."""
        rate = self._rate(sample_rate)
        if what not in ("logits", "scene", "frame", "segment", "segment_embeddings"):
            raise ValueError("what must be 'logits', 'scene', 'frame', 'segment' or 'segment_embeddings' (got %r)" % (what,))
        if what in ("segment", "segment_embeddings"):
            self._check_segment_call(pool)
        if isinstance(clips, torch.Tensor):
            if lengths is None:
                raise ValueError("a packed tensor needs `lengths`")
            if clips.dim() != 1:
                raise ValueError("expected a packed 1-D waveform tensor, got shape %r" % (tuple(clips.shape),))
            lengths = [int(n) for n in lengths]
            if sum(lengths) != clips.numel():
                raise ValueError("lengths sum to %d samples but the packed tensor holds %d" % (sum(lengths), clips.numel()))
            wav = clips
        else:
            clips = list(clips)
            if lengths is not None:
                raise ValueError("`lengths` goes with a packed tensor, not with a list of clips")
            for c in clips:
                if not isinstance(c, torch.Tensor) or c.dim() != 1:
                    raise ValueError("expected 1-D waveform tensors, got %r" % (getattr(c, "shape", type(c)),))
            lengths = [int(c.numel()) for c in clips]
            if not clips:
                raise ValueError("forward_varlen needs at least one clip")
            devs = {c.device for c in clips}
            if len(devs) != 1:
                raise RuntimeError("clips on several devices: %s" % sorted(str(d) for d in devs))
            self._check_run(clips[0].device)
            wav = torch.cat([c.detach().to(torch.float32) for c in clips])
        if not lengths:
            raise ValueError("forward_varlen needs at least one clip")
        self._check_run(wav.device)
        if rate is not None:
            for i, n in enumerate(lengths):
                _rs.check_min_length(n, rate, index=i)
            wav, lengths = _rs.resample(wav, rate, _rs.MODEL_RATE, lengths=lengths, _cache=self._resamplers)
        for i, n in enumerate(lengths):
            if n < _ffi.MIN_SAMPLES:
                raise RuntimeError("clip %d of %d samples is too short: kernel size can't be greater than actual input size "
                                   "(minimum is %d samples)" % (i, n, _ffi.MIN_SAMPLES))
        wav = wav.detach().to(torch.float32).contiguous()
        cap = _ffi.MAX_VARLEN_CLIPS
        parts, s0 = [], 0                 # (lengths of the call, out0, out1, clip)
        for c0 in range(0, len(lengths), cap):
            chunk = lengths[c0:c0 + cap]
            n = sum(chunk)
            parts.append((chunk,) + self._run_varlen(wav[s0:s0 + n], chunk, what, pool))
            s0 += n
        if what == "frame":
            views = []
            for chunk, buf, _, _ in parts:
                offs = varlen_frame_layout(chunk)
                for i in range(len(chunk)):
                    h3 = (offs[i + 1] - offs[i]) // (768 * 7)
                    views.append(buf[offs[i]:offs[i + 1]].view(768, h3, 7))
            return views
        if what in _ffi.SEG_WHAT:
            res = []
            for chunk, out0, out1, clip in parts:
                r0 = 0
                for i, L in enumerate(chunk):
                    r1 = r0 + _seg.segment_count(L)
                    if what == "segment":
                        res.append({"segmentwise_logits": out0[r0:r1], "segmentwise_output": out1[r0:r1],
                                    "clipwise_output": clip[i]})
                    else:
                        res.append(out0[r0:r1])
                    r0 = r1
            return res
        out0 = parts[0][1] if len(parts) == 1 else torch.cat([p[1] for p in parts])
        if what == "scene":
            return out0
        out1 = parts[0][2] if len(parts) == 1 else torch.cat([p[2] for p in parts])
        return {"clipwise_output": out1, "clipwise_logits": out0}

    def forward_windows(self, recordings, window=10.0, hop=None, what="logits", sample_rate=None, max_batch=64,
                        timeline="mean", pool=3):
        """Sliding-window tagging of long recordings (pytorch/windows.py has the definition).  Every window's outputs are
        bit-identical to the uniform forward of that window cut out and run alone.

        recordings: one 1-D CUDA tensor (returns one dict) or a list of them (returns a list of dicts).  window / hop: seconds,
        whole numbers of samples at 32 kHz; hop=None means hop = window.  Each dict has "starts" (float64 CPU tensor, window
        starts in seconds) and, by `what`: "logits" -> "clipwise_output" / "clipwise_logits" (n, N) plus "timeline"
        (ceil(L / hop), N), the per-step mean or max of the probabilities over the windows covering the step's midpoint
        (timeline="mean" | "max" | None); "scene" -> "scene" (n, 768); "frame" -> "frame" (n, 768, T', 7).  Recordings longer
        than the window run max_batch windows per call (acx_forward_windows); shorter ones are one window, the clip itself
        (forward_varlen).  what="segment" (forward_segments with `pool` on every window) -> "segmentwise_logits" /
        "segmentwise_output" (n, S_W, N), "clipwise_output" (n, N) and "timeline" at SEGMENT resolution: ceil(L / 10240) rows of
        0.32 s, row k the mean or max over the windows covering its midpoint of the one segment of each that holds it
        (pytorch/segments.py, segment_timeline_cover) -- with hop = window a gap-free 0.32 s timeline for one forward per
        window; "segment_embeddings" -> "segment_embeddings" (n, S_W, 768).  A recording not longer than the window gives one
        block of its own S rows.  sample_rate: the recordings' rate; they are resampled to 32 kHz on the device first (acx_resample)
        and the starts stay in seconds of the original audio."""
        rate = self._rate(sample_rate)
        if what not in ("logits", "scene", "frame", "segment", "segment_embeddings"):
            raise ValueError("what must be 'logits', 'scene', 'frame', 'segment' or 'segment_embeddings' (got %r)" % (what,))
        if what in ("segment", "segment_embeddings"):
            self._check_segment_call(pool)
        if timeline not in ("mean", "max", None):
            raise ValueError("timeline must be 'mean', 'max' or None (got %r)" % (timeline,))
        if isinstance(max_batch, bool) or not isinstance(max_batch, int) or max_batch < 1:
            raise ValueError("max_batch must be a positive integer (got %r)" % (max_batch,))
        W = _win.seconds_to_samples(window, "window")
        H = W if hop is None else _win.seconds_to_samples(hop, "hop")
        _win.check_window(W, H)
        single = isinstance(recordings, torch.Tensor)
        recs = [recordings] if single else list(recordings)
        if not recs:
            raise ValueError("forward_windows needs at least one recording")
        for r in recs:
            if not isinstance(r, torch.Tensor) or r.dim() != 1:
                raise ValueError("expected 1-D waveform tensors, got %r" % (getattr(r, "shape", type(r)),))
        devs = {r.device for r in recs}
        if len(devs) != 1:
            raise RuntimeError("recordings on several devices: %s" % sorted(str(d) for d in devs))
        self._check_run(recs[0].device)
        lengths = [int(r.numel()) for r in recs]
        wav = recs[0].detach() if len(recs) == 1 else torch.cat([r.detach().to(torch.float32) for r in recs])
        wav = wav.to(torch.float32).contiguous()
        if rate is not None:
            wav, lengths = _rs.resample(wav, rate, _rs.MODEL_RATE, lengths=lengths, _cache=self._resamplers)
        for i, n in enumerate(lengths):
            if n < _ffi.MIN_SAMPLES:
                raise RuntimeError("recording %d of %d samples at %d Hz is too short: kernel size can't be greater than actual "
                                   "input size (minimum is %d samples)" % (i, n, _rs.MODEL_RATE, _ffi.MIN_SAMPLES))
        offs = [0]
        for n in lengths:
            offs.append(offs[-1] + n)
        # by kind: the dict keys of (out0, out1, clip), and what the timeline steps over (None: the kind has no timeline)
        keys, tl_call, step = {
            "logits": (("clipwise_logits", "clipwise_output", None), "acx_window_timeline_classes", H),
            "scene": (("scene", None, None), None, None),
            "frame": (("frame", None, None), None, None),
            "segment": (("segmentwise_logits", "segmentwise_output", "clipwise_output"), "acx_segment_timeline",
                        _seg.SEGMENT_SAMPLES),
            "segment_embeddings": (("segment_embeddings", None, None), None, None)}[what]
        results = []
        cap = _ffi.MAX_VARLEN_CLIPS
        for c0 in range(0, len(lengths), cap):
            idx = range(c0, min(c0 + cap, len(lengths)))
            long_ = [i for i in idx if lengths[i] > W]
            short = [i for i in idx if lengths[i] <= W]
            per = {}                  # recording -> its windows' (out0, out1 or None, clip or None)
            if long_:
                if long_ == list(range(long_[0], long_[-1] + 1)):        # back to back in wav already: no copy
                    packed = wav[offs[long_[0]]:offs[long_[-1] + 1]]
                else:
                    packed = torch.cat([wav[offs[i]:offs[i + 1]] for i in long_])
                outs = self._run_windows(packed, [lengths[i] for i in long_], W, H, what, max_batch, pool)
                w0 = 0
                for i in long_:
                    n = _win.window_count(lengths[i], W, H)
                    per[i] = tuple(None if t is None else t[w0:w0 + n] for t in outs)
                    w0 += n
            if short:                 # one window each, the clip itself: forward_varlen's per-clip results as blocks of one window
                res = self.forward_varlen([wav[offs[i]:offs[i + 1]] for i in short], what=what, pool=pool)
                for k, i in enumerate(short):
                    if what == "logits":
                        per[i] = (res["clipwise_logits"][k:k + 1], res["clipwise_output"][k:k + 1], None)
                    elif what == "scene":
                        per[i] = (res[k:k + 1], None, None)
                    elif what == "segment":
                        per[i] = tuple(res[k][key][None] for key in keys)
                    else:
                        per[i] = (res[k][None], None, None)
            tl = None
            if tl_call is not None and timeline is not None:
                n_cls = per[idx[0]][1].shape[-1]
                probs = torch.cat([per[i][1].reshape(-1, n_cls) for i in idx]).contiguous()
                chunk = [lengths[i] for i in idx]
                tl = torch.empty((sum((n + step - 1) // step for n in chunk), n_cls), dtype=torch.float32, device=wav.device)
                lens = (ctypes.c_int64 * len(chunk))(*chunk)
                with torch.cuda.device(wav.device):
                    _ffi.check(getattr(_ffi.lib(), tl_call)(_ffi.ptr(probs), n_cls, lens, len(chunk), W, H,
                                                            1 if timeline == "max" else 0, _ffi.ptr(tl),
                                                            _ffi.stream_ptr(wav.device)))
            t0 = 0
            for i in idx:
                starts = _win.window_starts([lengths[i]], W, H)
                d = {"starts": torch.tensor(starts, dtype=torch.float64) / _rs.MODEL_RATE}
                d.update((key, t) for key, t in zip(keys, per[i]) if key is not None)
                if tl is not None:
                    steps = (lengths[i] + step - 1) // step
                    d["timeline"] = tl[t0:t0 + steps]
                    t0 += steps
                results.append(d)
        return results[0] if single else results

    def stream(self, slots=256, window=10.0, hop=1.0, what="logits", sample_rate=None, timeline="mean", max_push=2.0,
               max_batch=64, events=None, event_source="windows"):
        """A live-stream handle (pytorch/stream.py): `slots` recordings pushed chunk by chunk, each tagged window by window as
        soon as a window is complete, with the bits of forward_windows over the whole recording for any chunking.
        st.push(chunks) -- a list of `slots` 1-D CUDA tensors or None, or {slot: tensor} -- and st.close(slots=None) return
        one flat dict per call: "slot" / "starts" (CPU) and, by `what`, the outputs of the windows emitted by the call;
        "timeline" / "timeline_slot" / "timeline_step" for the rows that became final (logits with a timeline; a row trails the
        newest window by about one window length); "short": the slots whose recording ended under the model's minimum
        length and emitted nothing.  window / hop: seconds, whole samples at 32 kHz; sample_rate: the input rate of every
        slot; max_push: the longest chunk the device state is sized for, in seconds -- a longer one is pushed in pieces;
        max_batch: windows per forward.  Segment outputs (forward_segments) are not part of live streams: run
        forward_windows(what="segment") on the finished recording.
        events: a dict of decode_events' threshold / low / median / min_duration / merge_gap (what="logits" only) -- the
        handle then decodes sound events live, one step per hop, with an online decoder whose state lives on the device
        (segments.EventStream): every push() / close() dict gains "events", the EventTable (clip = slot, begin / end in hops
        of the slot's recording) of the events this call made final, each handed out once, and "events_open", (n, N) int32
        per slot touched (ascending) and class the step at which the event the class is inside of began, or -1.
        event_source="windows": row j is window j's "clipwise_output"; detection lags the audio by one window plus
        median // 2 hops plus merge_gap -- the low-latency form.  "timeline": the rows are the timeline's (needs timeline=)
        and inherit its trail; the last boundary is the end of the audio.  Over all calls a recording's events are
        decode_events_gpu of forward_windows' rows of the whole recording, byte for byte.  close() reads the last push's event
        count before it ends the recordings (one small synchronisation)."""
        return _stream.Stream(self, slots=slots, window=window, hop=hop, what=what, sample_rate=sample_rate,
                              timeline=timeline, max_push=max_push, max_batch=max_batch, events=events,
                              event_source=event_source)

    def fit_head(self, data, target, sample_rate=None, augment=None, views=1, mixup_alpha=None, **kw):
        """Train a new classifier head on this (frozen) backbone and install it (pytorch/finetune.py, fit_head): `data` is an
        (n, 768) tensor of scene embeddings, or a list of waveforms at `sample_rate`, whose scene embeddings are extracted
        first (extract(..., what="scene", pack=True)); target: (n, N) bool / uint8 / float labels; **kw: fit_head's settings
        (loss="ce", classes=N with (n,) integer labels trains a single-label head; read it with classify()).
        Afterwards head_audioset is an nn.Linear(768, N) with the fitted weights on the model's device -- the next forward
        runs it, state_dict() saves a checkpoint that from_pretrained loads as a fine-tuned model.  The model stays in eval
        mode.  Returns the HeadFit.
        augment: an augment.AugmentPolicy -- the head is then fitted on `views` augmented passes over the clips
        (augment.augmented_embeddings with seed = the fit's `seed`, mixup_alpha mixing clips and label rows pairwise), as the
        reference fine-tunes; `data` must be waveforms of one length.  The fit itself is the same fit_head on those rows."""
        from . import finetune as _ft
        emb, target = self._fit_inputs(data, target, sample_rate, augment, views, mixup_alpha, kw.get("seed", 0))
        fit = _ft.fit_head(emb, target, **kw)
        self._install_fit(fit)
        return fit

    def fit_sed_head(self, data, target, pooling="max", pool=3, sample_rate=None, **kw):
        """Train a sound event detection head from CLIP-level labels on this (frozen) backbone and install it
        (pytorch/finetune.py, fit_sed_head): the head sees every 0.32 s segment embedding, the segment probabilities are pooled
        over the clip (`pooling`: "max" -- what forward_segments' "clipwise_output" and detect_events read --, "mean", "linear",
        "exp") and the loss is taken on the pooled probability: the path detect_events / psds take at inference, which a
        fit_head on scene embeddings never sees.  data: waveforms at `sample_rate` -- a (B, L) tensor or a list of 1-D clips of
        any lengths, whose segment embeddings are computed with the `pool` that detection will use (forward_segment_embeddings /
        forward_varlen(what="segment_embeddings")) -- or segment embeddings as finetune.fit_sed_head takes them ((B, S, 768), a
        list of (S_i, 768), (packed, lengths)); target: (clips, N); **kw: fit_sed_head's settings.  The head is installed as
        fit_head installs its own; the model stays in eval mode.  Returns the HeadFit."""
        from . import finetune as _ft
        _ft.check_pooling(pooling)
        dev = self.head_audioset.weight.device
        is_emb = ((isinstance(data, torch.Tensor) and data.dim() == 3)
                  or (isinstance(data, tuple) and len(data) == 2 and isinstance(data[0], torch.Tensor) and data[0].dim() == 2
                      and data[0].shape[1] == _ft.EMBED_DIM and not (isinstance(data[1], torch.Tensor) and data[1].dim() == 2))
                  or (isinstance(data, (list, tuple)) and len(data) > 0
                      and all(isinstance(d, torch.Tensor) and d.dim() == 2 for d in data)))
        if is_emb:
            segments = data
        else:
            self._check_segment_call(pool)
            with torch.no_grad():
                if isinstance(data, torch.Tensor):
                    segments = self.forward_segment_embeddings(data.to(dev), pool=pool, sample_rate=sample_rate)
                else:
                    clips = [torch.as_tensor(c, dtype=torch.float32).to(dev) for c in data]
                    segments = [s.clone() for s in self.forward_varlen(clips, what="segment_embeddings", sample_rate=sample_rate,
                                                                       pool=pool)]
        if isinstance(target, torch.Tensor) and target.device != dev:
            target = target.to(dev)
        fit = _ft.fit_sed_head(segments, target, pooling=pooling, **kw)
        self._install_fit(fit)
        return fit

    def cross_validate_head(self, data, target, sample_rate=None, install=True, augment=None, views=1, mixup_alpha=None, **kw):
        """k-fold cross-validation of a new head over a grid of settings (pytorch/finetune.py, cross_validate_head): data and
        target exactly as fit_head takes them; **kw: folds=, grid=, fold_ids=, stratify=, metric=, refit= and fit_head's
        settings.  install=True installs cv.final -- the best setting refitted on all rows -- as fit_head installs its fit
        (nothing is installed with refit=False).  augment / views / mixup_alpha: as fit_head takes them; the folds are cut over
        the augmented rows.  Returns the CrossValidation."""
        from . import finetune as _ft
        emb, target = self._fit_inputs(data, target, sample_rate, augment, views, mixup_alpha, kw.get("seed", 0))
        cv = _ft.cross_validate_head(emb, target, **kw)
        if install and cv.final is not None:
            self._install_fit(cv.final)
        return cv

    def _fit_inputs(self, data, target, sample_rate, augment=None, views=1, mixup_alpha=None, seed=0):
        from .extract_embeddings import extract
        dev = self.head_audioset.weight.device
        if augment is None and (views != 1 or mixup_alpha is not None):
            raise ValueError("views= and mixup_alpha= go with augment= (an AugmentPolicy; AugmentPolicy.identity() for mixup alone)")
        if augment is not None:
            from . import augment as _aug
            if isinstance(data, torch.Tensor) and data.dim() == 2 and data.shape[1] == 768:
                raise ValueError("augment= needs waveform input: the augmentations act on the audio and its log-mel, and an "
                                 "(n, 768) embedding tensor has neither")
            if not isinstance(target, torch.Tensor):
                target = torch.as_tensor(target)
            return _aug.augmented_embeddings(self, data, target.to(dev), augment, views=views, mixup_alpha=mixup_alpha, seed=seed,
                                             sample_rate=sample_rate)
        if isinstance(data, torch.Tensor) and data.dim() == 2:
            emb = data
        else:
            emb = torch.stack(extract(self, list(data), what="scene", pack=True, sample_rate=sample_rate)).to(dev)
        if isinstance(target, torch.Tensor) and target.device != emb.device:
            target = target.to(emb.device)
        return emb, target

    def _install_fit(self, fit):
        from . import finetune as _ft
        dev = self.head_audioset.weight.device
        head = nn.Linear(_ft.EMBED_DIM, fit.weight.shape[0]).to(dev)
        with torch.no_grad():
            head.weight.copy_(fit.weight)
            head.bias.copy_(fit.bias)
        head.train(self.training)
        self.head_audioset = head

    def calibrate(self, data, target, method="platt", sample_rate=None, **kw):
        """Fit a calibration map for this model's head on a validation split (pytorch/calibration.py): `data` is an (n, N)
        tensor of clipwise_logits, or a list of waveforms at `sample_rate`, whose logits are extracted first
        (extract(..., what="logits", pack=True), as fit_head extracts embeddings).  method="platt": target (n, N) 0 / 1 labels
        -> PlattScaling (tag(calibration=)); method="temperature": target (n,) class numbers -> TemperatureScaling
        (classify(calibration=)).  **kw: smooth= / evaluations=.  Nothing is installed in the model."""
        from . import calibration as _cal
        from .extract_embeddings import extract
        if method not in ("platt", "temperature"):
            raise ValueError("method must be \"platt\" or \"temperature\" (got %r)" % (method,))
        dev = self.head_audioset.weight.device
        if isinstance(data, torch.Tensor) and data.dim() == 2:
            logits = data.to(dev)
        else:
            logits = torch.stack(extract(self, list(data), what="logits", pack=True, sample_rate=sample_rate)).to(dev)
        if isinstance(target, torch.Tensor) and target.device != logits.device:
            target = target.to(logits.device)
        if method == "platt":
            return _cal.fit_platt(target, logits, **kw)
        return _cal.fit_temperature(target, logits, **kw)

    def build_index(self, data, target=None, sample_rate=None, metric="cosine", quantize=None, rerank=True, oversample=4):
        """An EmbeddingIndex (pytorch/retrieval.py) over scene embeddings on the model's device: `data` is an (n, 768) tensor
        of embeddings, or a list of waveforms at `sample_rate`, whose scene embeddings are extracted first
        (extract(..., what="scene", pack=True), as fit_head does); target: optional (n, C) labels for idx.classify.
        quantize="int8": a QuantizedIndex instead -- the coarse search on int8 codes, with rerank=True followed by the exact
        fp32 scores of k * oversample candidates."""
        from .extract_embeddings import extract
        from .retrieval import EmbeddingIndex, QuantizedIndex
        if quantize not in (None, "int8"):
            raise ValueError("quantize must be None or \"int8\", got %r" % (quantize,))
        dev = self.head_audioset.weight.device
        if getattr(data, "ndim", None) == 2:
            emb = data
        else:
            emb = torch.stack(extract(self, list(data), what="scene", pack=True, sample_rate=sample_rate)).to(dev)
        if quantize == "int8":
            return QuantizedIndex(emb, metric=metric, target=target, device=dev, rerank=rerank, oversample=oversample)
        return EmbeddingIndex(emb, metric=metric, target=target, device=dev)

    def cluster(self, data, clusters, sample_rate=None, **kw):
        """K-means (pytorch/clustering.py: kmeans) over scene embeddings on the model's device: `data` is an (n, 768) tensor of
        embeddings, or a list of waveforms at `sample_rate`, extracted as build_index does; kw: metric, init, n_init, max_iter,
        tol, seed.  -> clustering.KMeans."""
        from .clustering import kmeans
        from .extract_embeddings import extract
        dev = self.head_audioset.weight.device
        if getattr(data, "ndim", None) == 2:
            emb = data
        else:
            emb = torch.stack(extract(self, list(data), what="scene", pack=True, sample_rate=sample_rate)).to(dev)
        return kmeans(emb, clusters, device=dev, **kw)

    def select_clusters(self, data, ks, sample_rate=None, **kw):
        """Choose the number of clusters (pytorch/cluster_scores.py: select_clusters) over scene embeddings on the model's device:
        `data` as cluster() takes it, one k-means fit per k of `ks`, each scored on the device; kw: criterion, metric, sample,
        seed and the k-means arguments.  -> cluster_scores.ClusterSelection (scores, best_k, best, fits)."""
        from .cluster_scores import select_clusters
        return select_clusters(self._scene_rows(data, sample_rate), ks, device=self.head_audioset.weight.device, **kw)

    def find_duplicates(self, data, threshold=0.95, sample_rate=None, **kw):
        """The groups of near-duplicate clips (pytorch/neighbors.py: duplicate_groups) over scene embeddings on the model's device:
        `data` as cluster() takes it; kw: metric, max_rounds.  -> neighbors.DuplicateGroups (labels, sizes, keep, pairs, groups())."""
        from .neighbors import duplicate_groups
        return duplicate_groups(self._scene_rows(data, sample_rate), threshold, device=self.head_audioset.weight.device, **kw)

    def dbscan(self, data, eps, min_samples=5, sample_rate=None, **kw):
        """Density clustering (pytorch/neighbors.py: dbscan) over scene embeddings on the model's device: `data` as cluster() takes
        it; kw: metric, max_rounds.  -> neighbors.DBSCANResult (labels with -1 for noise, core, counts, clusters)."""
        from .neighbors import dbscan
        return dbscan(self._scene_rows(data, sample_rate), eps, min_samples, device=self.head_audioset.weight.device, **kw)

    def fit_gmm(self, data, components, sample_rate=None, **kw):
        """A Gaussian mixture (pytorch/mixture.py: gmm) over scene embeddings on the model's device: `data` as cluster() takes it;
        kw: covariance_type, init, n_init, max_iter, tol, reg_covar, seed and the *_init arguments.  -> mixture.GaussianMixture
        (score_samples is the anomaly score of new clips)."""
        from .mixture import gmm
        return gmm(self._scene_rows(data, sample_rate), components, device=self.head_audioset.weight.device, **kw)

    def select_components(self, data, ks, sample_rate=None, **kw):
        """Choose the number of mixture components by BIC or AIC (pytorch/mixture.py: select_components) over scene embeddings on
        the model's device: `data` as cluster() takes it, one fit per k of `ks`; kw: criterion and the gmm arguments.
        -> mixture.ComponentSelection (scores, best_k, best, fits)."""
        from .mixture import select_components
        return select_components(self._scene_rows(data, sample_rate), ks, device=self.head_audioset.weight.device, **kw)

    def _scene_rows(self, data, sample_rate):
        """`data` as build_index takes it -> (n, 768) scene embeddings: a 2-D tensor of embeddings as it is, a list of waveforms
        at `sample_rate` extracted first (extract(..., what="scene", pack=True))."""
        from .extract_embeddings import extract
        if getattr(data, "ndim", None) == 2:
            return data
        return torch.stack(extract(self, list(data), what="scene", pack=True, sample_rate=sample_rate)).to(self.head_audioset.weight.device)

    def frechet_distance(self, data_a, data_b, sample_rate=None, **kw):
        """The Frechet (audio) distance between two sets on the model's device (pytorch/statistics.py: frechet_distance): each
        of data_a / data_b is an (n, 768) tensor of scene embeddings, or a list of waveforms at `sample_rate`, extracted as
        build_index does; kw: max_sweeps.  -> statistics.FrechetDistance (0-d device tensors; float() / check() synchronise)."""
        from .statistics import frechet_distance
        a, b = self._scene_rows(data_a, sample_rate), self._scene_rows(data_b, sample_rate)
        return frechet_distance(a, b, device=self.head_audioset.weight.device, **kw)

    def fit_pca(self, data, components=None, whiten=False, sample_rate=None, **kw):
        """PCA (pytorch/statistics.py: PCA.fit) of scene embeddings on the model's device: `data` is an (n, 768) tensor of
        embeddings, or a list of waveforms at `sample_rate`; components: None, an integer, or a float in (0, 1) = the share of
        the variance to keep; kw: max_sweeps, eps.  -> statistics.PCA."""
        from .statistics import PCA
        return PCA.fit(self._scene_rows(data, sample_rate), components, whiten, device=self.head_audioset.weight.device, **kw)

    def search(self, index, waveform, k=10, sample_rate=None):
        """Query by example: {"scores" (B, k) fp32, "indices" (B, k) int64, "scene" (B, 768)} of a (B, L) waveform batch --
        forward_scene_embeddings, then index.search, on one stream with no host synchronisation (capturable as a whole).
        index.check() reports a NaN or infinity met on the way."""
        scene = self.forward_scene_embeddings(waveform, sample_rate=sample_rate)
        scores, indices = index.search(scene, k=k)
        return {"scores": scores, "indices": indices, "scene": scene}

    # ----------------------------------------------------------------------------- public surface
    # sample_rate (all three): the rate of x; None or 32000 is the model's own.  Any other integer rate is resampled to 32 kHz
    # on x's stream first (acx_resample, the interpolation of torchaudio.functional.resample that the reference's demo runs on
    # the host, demo_convnext.py:53-59); the result equals the forward of pytorch.resample.resample(x, sample_rate) bit for bit.
    def forward(self, x, mixup_lambda=None, sample_rate=None):
        """(B, L) waveform -> {"clipwise_output": probs, "clipwise_logits": logits}, each (B, N) (convnext.py:287-331)."""
        logits, probs, _ = self._run(self._resampled(x, sample_rate), "logits")
        return {"clipwise_output": probs, "clipwise_logits": logits}

    def forward_scene_embeddings(self, x, mixup_lambda=None, sample_rate=None):
        """(B, L) -> (B, 768) (convnext.py:333-366)."""
        return self._run(self._resampled(x, sample_rate), "scene")[0]

    def forward_frame_embeddings(self, x, mixup_lambda=None, sample_rate=None):
        """(B, L) -> NCHW (B, 768, T', 7) (convnext.py:369-402)."""
        return self._run(self._resampled(x, sample_rate), "frame")[0]

    def forward_augmented(self, x, policy=None, plan=None, mixup_lambda=None, what="logits", generator=None, sample_rate=None):
        """One forward with the reference's TRAINING-mode input transforms, the model in eval mode -- the backbone is frozen, the
        transforms are what a fine-tuning epoch of the reference sees (pytorch/augment.py has the definitions): gain, roll and
        speed perturbation of the waveform (convnext.py:288-295), SpecAugment stripes on the bn0'd log-mel (:308-309), mixup of
        clips 2b and 2b + 1 (:312-313).  All of it runs on x's stream (acx_forward_augmented), nothing synchronises after the
        plan's upload.
        policy: an augment.AugmentPolicy (None: AugmentPolicy.reference(), SpecAugment only), drawn with `generator` (a torch
        CPU generator; None: the global one); or plan: an augment.AugmentPlan drawn earlier (policy and generator unused).
        mixup_lambda: B values (the reference's argument; B even) -- the outputs then have B / 2 rows.
        what: "logits" -> {"clipwise_output", "clipwise_logits"}; "scene" -> {"scene": (rows, 768)}; "frame" -> {"frame":
        (rows, 768, T', 7)}; each dict also has "plan", the AugmentPlan that was applied.  With AugmentPolicy.identity() and
        no lambdas the outputs equal model(x) / forward_scene_embeddings / forward_frame_embeddings bit for bit."""
        from . import augment as _aug
        if what in _ffi.SEG_WHAT:
            raise ValueError("forward_augmented has no segment outputs (what=%r): the augmented forwards are logits, scene and "
                             "frame" % (what,))
        if what not in _ffi.MODES:
            raise ValueError("what must be 'logits', 'scene' or 'frame' (got %r)" % (what,))
        x = self._resampled(x, sample_rate)
        self._check_batch(x)
        self._check_run(x.device)
        x = x.detach().to(torch.float32).contiguous()
        B, L = x.shape
        if L < _ffi.MIN_SAMPLES:
            raise RuntimeError("clip of %d samples is too short: kernel size can't be greater than actual input size "
                               "(minimum is %d samples)" % (L, _ffi.MIN_SAMPLES))
        if plan is None:
            plan = _aug.draw_plan(_aug.AugmentPolicy.reference() if policy is None else policy, B, L, generator)
        elif not isinstance(plan, _aug.AugmentPlan) or (plan.B, plan.L) != (B, L):
            raise ValueError("plan must be an AugmentPlan of this batch (%d clips of %d samples)" % (B, L))
        dev = x.device
        lam = None
        if mixup_lambda is not None:
            lam = torch.as_tensor(mixup_lambda).detach().to(torch.float32).reshape(-1).contiguous()
            lam = (lam if lam.is_cuda else lam.pin_memory()).to(dev, non_blocking=True)
            if B % 2 or lam.numel() != B:
                raise ValueError("mixup pairs clips 2b and 2b + 1: %d clips with %d lambdas (expected an even batch and one "
                                 "lambda per clip)" % (B, lam.numel()))
        rows = B // 2 if lam is not None else B
        dplan = plan.to(dev)
        with torch.cuda.device(dev):
            ctx = self.native_context(dev)
            ws = self._workspace(dev, ctx.workspace_bytes_augmented(B, L, dplan.wave_dev is not None, lam is not None, what))
            out0, out1, _ = self._outputs(what, (rows,), ctx.classes, L, dev)
            _ffi.check(_ffi.lib().acx_forward_augmented(ctx.handle, _ffi.ptr(x), B, L, _ffi.ptr(dplan.wave_dev),
                                                        _ffi.ptr(dplan.spec_dev), _ffi.ptr(lam), _ffi.MODES[what], _ffi.ptr(out0),
                                                        _ffi.ptr(out1), _ffi.ptr(ws), ws.numel(), _ffi.stream_ptr(dev)))
        if what == "logits":
            return {"clipwise_output": out1, "clipwise_logits": out0, "plan": plan}
        return {what: out0, "plan": plan}

    @classmethod
    def from_pretrained(cls, pretrained_checkpoint_path, map_location=None, use_auth_token=None):
        """Local file first, then a Zenodo URL, then a Hugging Face model id[@revision]
        (convnext.py:404-511).  Accepts both `model.safetensors` and the `.pth` ({"model": sd}) form that
        evaluate_convnext_on_audioset.py:36-38 loads; the head is sized from the checkpoint's `head_audioset.weight` (527 rows
        for AudioSet, N for a fine-tuned model).  Returns None when the HF repo does not exist."""
        if os.path.isfile(pretrained_checkpoint_path):
            print("Ckpt already on local disk")
            path_ = pretrained_checkpoint_path
        elif "https" in pretrained_checkpoint_path:
            print("Using ckpt from Zenodo")
            dpath_ = os.path.join(torch.hub.get_dir(), "checkpoints")
            os.makedirs(dpath_, exist_ok=True)
            fname = os.path.basename(pretrained_checkpoint_path).replace("?download=1", "")
            path_ = os.path.join(dpath_, fname)
            torch.hub.download_url_to_file(pretrained_checkpoint_path, path_)
        else:
            print("Using ckpt from HF")
            from huggingface_hub import hf_hub_download
            from huggingface_hub.utils import RepositoryNotFoundError
            model_id, _, revision = pretrained_checkpoint_path.partition("@")
            try:
                path_ = hf_hub_download(model_id, HF_PYTORCH_WEIGHTS_NAME, repo_type="model",
                                        revision=revision or None, library_name="audioset-convnext",
                                        token=use_auth_token)
            except RepositoryNotFoundError:
                print("\nCould not download '%s' model.\nIt might be because the model is private or gated so make\n"
                      "sure to authenticate. Visit https://hf.co/settings/tokens to\ncreate your access token and "
                      "retry with use_auth_token=YOUR_AUTH_TOKEN" % model_id)
                return None
            try:        # the hub's download counter keys on config.yaml (convnext.py:470-493)
                hf_hub_download(model_id, HF_CONFIG_NAME, repo_type="model", revision=revision or None,
                                library_name="audioset-convnext", token=use_auth_token)
            except Exception:
                pass
        model = convnext_tiny(pretrained=False, strict=False, drop_path_rate=0.0, after_stem_dim=[252, 56],
                              use_speed_perturb=False)
        load_checkpoint(model, path_, map_location or "cpu")
        return model


def varlen_frame_layout(lengths):
    """Element offsets of the clips' (768, T'_i, 7) blocks in the frame output of acx_forward_varlen: B + 1 ascending values,
    the last one the buffer's size.  T' follows acx_stage_hw: T = L // 320 + 1, H0 = (T + 4) // 4 + 1, T' = H0 // 8."""
    offs = [0]
    for L in lengths:
        h0 = (int(L) // 320 + 1 + 4) // 4 + 1
        offs.append(offs[-1] + 768 * (h0 // 2 // 2 // 2) * 7)
    return offs


def check_num_classes(n):
    """The class counts a classifier head may have: 1 .. 32768 (ACX_MAX_CLASSES)."""
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= _ffi.MAX_CLASSES:
        raise ValueError("num_classes must be an integer in [1, %d] (got %r)" % (_ffi.MAX_CLASSES, n))
    return n


def _size_head(model, shape):
    """Give `model` a fresh nn.Linear(768, N) head when the checkpoint's head_audioset.weight has N rows and the model's has not
    (a fine-tuned checkpoint); its values come from the checkpoint right after."""
    if shape is None or len(shape) != 2:
        return
    n = int(shape[0])
    if n != model.head_audioset.out_features:
        check_num_classes(n)
        dev = model.head_audioset.weight.device
        model.head_audioset = nn.Linear(int(shape[1]), n).to(dev)


def load_checkpoint(model, path, map_location="cpu"):
    """`.safetensors` via safetensors.torch.load_model (strict, convnext.py:507); anything else as a torch
    checkpoint holding {"model": state_dict} (evaluate_convnext_on_audioset.py:36-38).  The head is sized from the
    checkpoint's `head_audioset.weight`: a 527-row checkpoint loads as before, an N-row one gives an N-class model."""
    if str(path).endswith(".safetensors"):
        from safetensors import safe_open
        from safetensors.torch import load_model as st_load_model
        with safe_open(str(path), framework="pt") as f:
            if "head_audioset.weight" in f.keys():
                _size_head(model, f.get_slice("head_audioset.weight").get_shape())
        st_load_model(model, path)
    else:
        ckpt = torch.load(path, map_location=map_location)
        sd = ckpt["model"] if "model" in ckpt else ckpt
        w = sd.get("head_audioset.weight")
        _size_head(model, None if w is None else tuple(w.shape))
        model.load_state_dict(sd)
    return model


def convnext_tiny(pretrained=False, strict=False, in_22k=False, drop_path_rate=0.1, after_stem_dim=[56],
                  use_speed_perturb=False, use_pydub_augment=False, use_roll_augment=False, **kwargs):
    """Same signature as the reference factory (convnext.py:641-708).  Only the configuration the
    reference's demo / evaluation / from_pretrained use is built: after_stem_dim=[252, 56], no ImageNet
    pre-training download.  `drop_path_rate` only matters in training and is ignored in eval."""
    if pretrained:
        raise NotImplementedError("ImageNet initialisation is a training feature (and needs network access)")
    if list(after_stem_dim) != [252, 56]:
        raise ValueError("ERROR: this build implements the after_stem_dim=[252,56] stem "
                         "(the one every shipped entry point of the reference uses)")
    return ConvNeXt(in_chans=1, num_classes=527, depths=[3, 3, 9, 3], dims=[96, 192, 384, 768],
                    drop_path_rate=0.0, use_speed_perturb=use_speed_perturb,
                    use_pydub_augment=use_pydub_augment, use_roll_augment=use_roll_augment, **kwargs)
