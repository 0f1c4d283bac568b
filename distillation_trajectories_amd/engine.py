"""Host-side driver of the HIP path: weight hand-off, time-bias tables, device-resident
reverse loops and metric post-processing.  PyTorch is used for device memory, streams and
host<->device copies only; all arithmetic on trajectories happens in csrc/ kernels.

Everything here raises if the HIP library is missing or a tensor is not on a CUDA(HIP)
device -- the product has no CPU path (the CPU restatement lives in oracle/ and is test-only).
"""
import collections
import ctypes
import math
import os
import sys
import types
from ctypes import c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

import numpy as np
import torch

from . import _hip
from ._hip import (COND_NONE, COND_ONE, COND_ZERO, RULE_ENGINE, RULE_MANAGER, RULE_PSAMPLE, HipLibraryError, check,
                   ptr, stream_ptr)

AUTOTUNE_MIN_ROWS = 16384       # batch_total*H*W from which a forward shape is worth tuning once
BLOCK_NAMES = ("enc1", "enc2", "enc3", "enc4", "bottleneck", "dec3", "dec2", "dec1")
_BLOCK_KEYS = ("time_mlp.weight", "time_mlp.bias",
               "conv1.weight", "conv1.bias", "norm1.weight", "norm1.bias", "norm1.running_mean", "norm1.running_var",
               "conv2.weight", "conv2.bias", "norm2.weight", "norm2.bias", "norm2.running_mean", "norm2.running_var",
               "residual_conv.weight", "residual_conv.bias")
_GLOBAL_KEYS = ("time_mlp.1.weight", "time_mlp.1.bias", "cond_emb.0.weight", "cond_emb.0.bias",
                "cond_emb.2.weight", "cond_emb.2.bias", "final.weight", "final.bias")


def _require_cuda(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HipLibraryError(f"{what} must be a CUDA(HIP) tensor: the MI355X path has no CPU fallback "
                              "(the CPU restatement lives in oracle/ and is for tests only)")


def sinusoid_frequencies(dim):
    """models.py:17-21: exp(arange(half) * -(ln 1e4 / (half-1+1e-8))) with torch's fp32 dtype path."""
    half = max(max(dim, 2) // 2, 1)
    return torch.exp(torch.arange(half) * -(math.log(10000) / (half - 1 + 1e-8)))


# (DT_PLAN_TABLE=file: another table, e.g. a candidate from tools/plan_search.py; DT_PLAN_TABLE= (empty): no table)
PLAN_TABLE = os.environ.get("DT_PLAN_TABLE", os.path.join(os.path.dirname(os.path.abspath(__file__)), "plans", "gfx950.json"))


class _Plans:
    """Launch plans (tile / split / kernel family per convolution of a forward shape).

    Results must not depend on which process runs them: by default a shape's plan is a pure function of the model and the
    shape -- the entry of the COMMITTED per-arch table ``plans/gfx950.json`` (measured once with
    ``tools/make_plan_table.py`` for the BASELINE shapes) or, for shapes the table does not hold, the library's
    deterministic heuristic.  Timing candidates in the process (``dt_unet_autotune``: its picks between near-equal
    candidates differ from run to run, which changes results at fp32-rounding level) is opt-in: ``DT_AUTOTUNE=1``, or
    ``tune=True`` on a call; ``DT_TUNE_CACHE=file`` then records what was measured so that later processes replay it.
    """
    _table = None
    _lock = None

    @classmethod
    def table(cls):
        if cls._table is None:
            import json
            try:
                with open(PLAN_TABLE) as f:
                    cls._table = json.load(f).get("plans", {})
            except (OSError, ValueError):
                cls._table = {}
        return cls._table

    @staticmethod
    def cache_path():
        return os.environ.get("DT_TUNE_CACHE") or None

    @staticmethod
    def cache_load():
        import json
        p = _Plans.cache_path()
        if not p:
            return None
        try:
            with open(p) as f:
                return json.load(f)
        except (OSError, ValueError):
            return {}

    @staticmethod
    def cache_store(key, plan):
        """Read-modify-replace under an exclusive lock file (several ranks may tune at once)."""
        import fcntl
        import json
        p = _Plans.cache_path()
        with open(p + ".lock", "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            cache = _Plans.cache_load() or {}
            cache[key] = plan
            tmp = f"{p}.{os.getpid()}.tmp"
            with open(tmp, "w") as f:
                json.dump(cache, f)
            os.replace(tmp, p)

    @staticmethod
    def digest(plan):
        import hashlib
        import json
        return hashlib.sha1(json.dumps(plan, sort_keys=True).encode()).hexdigest()[:10]


import weakref

_HANDLES = weakref.WeakKeyDictionary()      # nn.Module -> (weights key, UNetHandle)
_TRAIN_WARNED = weakref.WeakSet()
_FUSED_DEFAULT = True


def set_fused_default(on):
    """Whether small models (padded dims <= 32 / 64) at 16x16 take the fused whole-forward kernel (dt_fused.hip): applies to
    every handle cached on a module and to handles created later.  ``DT_NO_FUSED=1`` in the environment is the same switch
    at library level (read when a handle is created)."""
    global _FUSED_DEFAULT
    _FUSED_DEFAULT = bool(on)
    for _, h in list(_HANDLES.values()):
        h.set_fused(_FUSED_DEFAULT)


class _Split(collections.namedtuple("_Split", "B n_pass b_single tb_div mixed")):
    """The batch of one forward or sampler call, as BatchSplit of csrc/dt_batch.h: B images of which the first ``b_single`` take
    one pass and the others ``n_pass``; ``tb_div`` rows share a time-bias row.  ``mixed``: the call goes to the library's
    mixed-batch entry (which refuses ``b_single`` == 0 and ``b_single`` == B) and not to the plain one."""
    __slots__ = ()

    @property
    def rows(self):
        return self.n_pass * self.B - self.b_single * (self.n_pass - 1)


class UNetHandle:
    """Owns one ``dt_unet`` (packed weights in HBM) built from a module's state_dict."""

    def __init__(self, state_dict, device):
        self.lib = _hip.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise HipLibraryError("models must live on a CUDA(HIP) device; there is no CPU fallback")
        sd = {k: v.detach().to(device=self.device, dtype=torch.float32).contiguous()
              for k, v in state_dict.items() if v.dtype.is_floating_point}
        self.channels = sd["final.weight"].shape[0]
        self.temb_dim = sd["time_mlp.1.weight"].shape[0]
        self.dims = [sd[f"{n}.conv1.weight"].shape[0] for n in ("enc1", "enc2", "enc3", "enc4")]
        desc = _hip.UNetDesc(self.channels, (c_int32 * 4)(*self.dims), self.temb_dim)
        bt = (c_void_p * (_hip.N_BLOCKS * _hip.BT_COUNT))()
        for j, name in enumerate(BLOCK_NAMES):
            for i, key in enumerate(_BLOCK_KEYS):
                t = sd.get(f"{name}.{key}")
                bt[j * _hip.BT_COUNT + i] = t.data_ptr() if t is not None else None
        freqs = sinusoid_frequencies(self.temb_dim).to(self.device)
        gt = (c_void_p * _hip.GT_COUNT)(*[sd[k].data_ptr() for k in _GLOBAL_KEYS], freqs.data_ptr())
        h = c_void_p()
        with torch.cuda.device(self.device):
            check(self.lib.dt_unet_create(ctypes.byref(desc), bt, gt, stream_ptr(), ctypes.byref(h)), "dt_unet_create")
            torch.cuda.current_stream().synchronize()   # sd / freqs may be freed after this
        self.h = h
        self.tb_stride = self.lib.dt_unet_time_bias_stride(self.h)
        mode = os.environ.get("DT_PRECISION", "auto")
        check(self.lib.dt_unet_set_precision(self.h, {"fp32": 0, "split-bf16": 1, "auto": 2}[mode]), "dt_unet_set_precision")
        self._mode = mode
        self._shared_enc1 = os.environ.get("DT_NO_SHARED_ENC1") is None      # read by dt_unet_create
        self._ws = {}
        self._consts = {}
        self._plans = {}              # (rows, H, W, images, single-pass images) -> plan id ("table:<sha1>", "tuned:<sha1>", "heuristic", "pinned")
        self._split = {}              # (rows, H, W) -> (images, single-pass images) last named for it: see shape()
        self._head_fusion = True      # the library's switch as set_head_fusion left it (it has no getter)
        if not _FUSED_DEFAULT:
            self.set_fused(False)

    def __del__(self):
        try:
            h, self.h = getattr(self, "h", None), None
            if h and not sys.is_finalizing():    # at interpreter exit the HIP runtime may already be gone
                self.lib.dt_unet_destroy(h)
        except Exception:
            pass

    # ------------------------------------------------------------------ caching per nn.Module
    @staticmethod
    def for_module(module):
        """Handle cached on the module; rebuilt when any weight tensor was replaced or mutated.

        The HIP path is inference-only (BatchNorm running statistics, no dropout, no autograd): a module left in
        train mode -- the reference's samplers never call ``eval()`` themselves (utils/diffusion.py:102-212) --
        would give different numbers in the reference, so that is reported once per module."""
        tensors = list(module.parameters()) + list(module.buffers())
        _require_cuda(tensors[0], "model parameters")
        # (the cache lives beside the module, not in its __dict__: a module that has run on the HIP path can still be
        # deep-copied, pickled and torch.save()d like any other nn.Module)
        if module.training and module not in _TRAIN_WARNED:
            import warnings
            _TRAIN_WARNED.add(module)
            warnings.warn("distillation_trajectories_amd: the model is in train mode, but the HIP path is inference-only "
                          "(BatchNorm running statistics, dropout off); call model.eval() as the reference's callers do",
                          RuntimeWarning, stacklevel=3)
        key = tuple((v.data_ptr(), v._version) for v in tensors)
        cached = _HANDLES.get(module)
        if cached is None or cached[0] != key:
            cached = (key, UNetHandle(module.state_dict(), tensors[0].device))
            _HANDLES[module] = cached
        return cached[1]

    # ------------------------------------------------------------------ primitives
    def workspace(self, batch_total, H, W):
        """Scratch of one forward shape, one buffer PER STREAM: two streams may run the same handle concurrently
        (activations live in the workspace, so a shared buffer would be a silent race)."""
        key = (batch_total, H, W, torch.cuda.current_stream(self.device).cuda_stream)
        ws = self._ws.get(key)
        if ws is None:
            n = self.lib.dt_unet_workspace_bytes(self.h, batch_total, H, W)
            if n == 0:
                raise HipLibraryError(f"unsupported shape batch={batch_total} H={H} W={W} (H, W must be multiples of 16)")
            if len(self._ws) > 8:
                torch.cuda.synchronize(self.device)     # a buffer may still be in use on another stream
                self._ws.clear()
            ws = self._ws[key] = torch.empty(n, dtype=torch.uint8, device=self.device)
        return ws

    def set_precision(self, mode):
        """PREC_FP32 (exact fp32 MFMA), PREC_SPLIT_BF16 (3-plane bf16 split, 6 products) or PREC_AUTO."""
        check(self.lib.dt_unet_set_precision(self.h, int(mode)), "dt_unet_set_precision")
        self._mode = {0: "fp32", 1: "split-bf16", 2: "auto"}[int(mode)]
        self._plans.clear()               # the library drops its tuned shapes, pins included: choices are per arithmetic mode

    def set_fused(self, on):
        """Small models at 16x16: whole forward / whole sampler loop as one launch (dt_unet_set_fused); no-op for models
        that do not qualify."""
        check(self.lib.dt_unet_set_fused(self.h, int(bool(on))), "dt_unet_set_fused")

    def fused_active(self, H, W):
        return bool(self.lib.dt_unet_fused_active(self.h, H, W))

    def set_head_fusion(self, on):
        """Test hook (dt_unet_set_head_fusion): off = separate head launch, dec1's output is materialised."""
        check(self.lib.dt_unet_set_head_fusion(self.h, int(bool(on))), "dt_unet_set_head_fusion")
        self._head_fusion = bool(on)

    @property
    def _tuned(self):
        """{(rows, H, W)} of the shapes that run a table / measured / pinned plan (not the bare heuristic)."""
        return {k[:3] for k, v in self._plans.items() if v != "heuristic"}

    # version of the launch-plan vocabulary (tile sizes, launch kinds, split semantics of dt_unet_set_conv_choice): the committed
    # table and recorded caches stay valid across ABI revisions that only ADD entry points (ABI 4 added the fused-path switches)
    PLAN_VERSION = 3

    def plan_key(self, rows, H, W, imgs, single):
        return (f"abi{self.PLAN_VERSION}|gfx950|prec={self._mode}|enc1={'shared' if self._shared_enc1 else 'per-pass'}|C{self.channels}"
                f"|D{self.temb_dim}|{','.join(map(str, self.dims))}|{rows}x{H}x{W}|{imgs}/{single}")

    def shape(self, rows, H, W, imgs=None, single=0):
        """The full forward shape ``(rows, H, W, images, single-pass images)`` that keys a launch plan in the library and here.

        A call that names the split (``forward``, ``forward_mixed``, ``sample``, ``sample_mixed``, ``ensure_plan``,
        ``set_conv_choice(images=...)``) has it remembered for its ``(rows, H, W)``.  A call that names only the rows
        (``conv_choices``, ``set_conv_choice`` without ``images``, ``time_conv``, ``_read_plan``) means the split remembered
        last, else the sampler's two-pass split: ``rows // 2`` images when ``rows`` is even, ``rows`` images otherwise.
        This is the only memory of a "last shape" anywhere; ``set_precision`` does not clear it."""
        if imgs is None:
            imgs, single = self._split.get((rows, H, W), (rows // 2 if rows % 2 == 0 else rows, 0))
        else:
            self._split[(rows, H, W)] = (imgs, single)
        return (rows, H, W, imgs, single)

    def _choices(self, key):
        """(block, slot, bm, bn, splits, kind, skip folded, tuned) of every launch of a shape (dt_unet_conv_choice)."""
        for j in range(8):
            for slot in range(3):
                v = [c_int() for _ in range(5)]
                check(self.lib.dt_unet_conv_choice(self.h, *key, j, slot, *map(ctypes.byref, v)), "dt_unet_conv_choice")
                bm, bn, sp, pr, tu = (x.value for x in v)
                if bm:
                    yield j, slot, bm, bn, sp, pr & 7, 1 if pr & 8 else 0, bool(tu)

    def _read_plan(self, rows, H, W):
        return [list(c[:7]) for c in self._choices(self.shape(rows, H, W))]

    def _apply_plan(self, key, plan):
        """Pin every launch of a recorded plan; an entry this build no longer admits (or that contradicts the handle's
        arithmetic mode) is skipped, which leaves that slot on the heuristic."""
        ok = True
        for block, slot, bm, bn, sp, prec, fuse in plan:
            if (self._mode == "fp32") != (prec == _hip.KIND_FP32) and self._mode != "auto":
                ok = False
                continue
            if self.lib.dt_unet_set_conv_choice(self.h, *key, block, slot, bm, bn, sp, prec, fuse) != 0:
                ok = False
        return ok

    def ensure_plan(self, rows, H, W, imgs, single, tune=None, warm=None):
        """Settle the launch plan of a forward shape once (see ``_Plans``); a shape with launches pinned by hand
        (``set_conv_choice``) is left alone.  ``warm`` runs one forward of the shape (real activations in the workspace)
        before candidates are timed.  Returns the plan id."""
        key = self.shape(rows, H, W, imgs, single)
        have = self._plans.get(key)
        if have is not None and not (tune is True and not have.startswith(("tuned", "pinned"))):
            return have
        if tune is False:
            self._plans[key] = "heuristic"
            return "heuristic"
        pkey = self.plan_key(*key)
        if tune is not True:
            for source, entries in (("table", _Plans.table()), ("cache", _Plans.cache_load() or {})):
                plan = entries.get(pkey)
                if plan and self._apply_plan(key, plan):
                    self._plans[key] = f"{source}:{_Plans.digest(plan)}"
                    return self._plans[key]
        measure = tune is True or (os.environ.get("DT_AUTOTUNE", "0") == "1" and rows * H * W >= AUTOTUNE_MIN_ROWS)
        if not measure:
            self._plans[key] = "heuristic"
            return "heuristic"
        if warm is not None:
            warm()
        ws = self.workspace(rows, H, W)
        with torch.cuda.device(self.device):
            check(self.lib.dt_unet_autotune(self.h, *key, ptr(ws), c_size_t(ws.numel()), stream_ptr()), "dt_unet_autotune")
        plan = self._read_plan(rows, H, W)
        self._plans[key] = f"tuned:{_Plans.digest(plan)}"
        if _Plans.cache_path():
            _Plans.cache_store(pkey, plan)
        return self._plans[key]

    def plan_ids(self):
        """{"rowsxHxW imgs/single": plan id} of every shape this handle has run (bench.py prints it)."""
        return {f"{k[0]}x{k[1]}x{k[2]} {k[3]}/{k[4]}": v for k, v in sorted(self._plans.items())}

    def set_conv_choice(self, batch_total, H, W, block, slot, bm, bn, splits=1, prec=1, fuse=0, images=None, single=0):
        """Pin one convolution's launch choice for a forward shape (dt_unet_set_conv_choice); the shape's plan id becomes
        ``"pinned"``.  A launch pinned by hand asks for the layered kernels, so the handle leaves the fused small-model path
        (``set_fused(True)`` returns to it).

        A pin belongs to the full shape: ``images`` (with ``single``, the single-pass images of a mixed batch) names the split
        of the forward it is meant for, e.g. ``images=batch_total`` for a one-pass forward; without it, see ``shape``."""
        key = self.shape(batch_total, H, W, images, single)
        check(self.lib.dt_unet_set_conv_choice(self.h, *key, block, slot, bm, bn, splits, prec, fuse), "dt_unet_set_conv_choice")
        self.set_fused(False)
        self._plans[key] = "pinned"

    def conv_choices(self, batch_total, H, W):
        """[(block, slot, bm, bn, splits, kind, tuned)] for reporting."""
        return [(BLOCK_NAMES[j], ("skip", "conv1", "conv2")[slot], bm, bn, sp, _hip.KIND_NAMES.get(kind, "-") + ("+skip" if fold else ""), tuned)
                for j, slot, bm, bn, sp, kind, fold, tuned in self._choices(self.shape(batch_total, H, W))]

    def time_conv(self, batch_total, H, W, block, slot, bm, bn, splits=1, prec=1, fuse=0, reps=10, images=None, single=0):
        """(milliseconds, algorithmic flops) of one convolution launch of a forward shape under an explicit choice
        (dt_unet_time_conv: one warm launch, then the average of ``reps``), on the activations the last forward left in the
        workspace; None where the library refuses the choice."""
        ws = self.workspace(batch_total, H, W)
        ms, fl = c_float(), ctypes.c_double()
        with torch.cuda.device(self.device):
            st = self.lib.dt_unet_time_conv(self.h, *self.shape(batch_total, H, W, images, single), block, slot, bm, bn, splits, prec,
                                            fuse, reps, ptr(ws), c_size_t(ws.numel()), stream_ptr(), ctypes.byref(ms), ctypes.byref(fl))
        return (ms.value, fl.value) if st == 0 else None

    def time_bias(self, t_values, cond_modes):
        """[rows, tb_stride] table for rows (t_values[i], cond_modes[i]); cond mode in {NONE, ZERO, ONE}.

        The three small index tensors are uploaded once per distinct row list and kept with the handle: a pageable
        host-to-device copy blocks the host until the stream has drained, which would stop a caller from queueing one
        sampler loop behind another."""
        rows = len(t_values)
        key = ("tb_in", tuple(int(v) for v in t_values), tuple(int(m) for m in cond_modes))
        cached = self._consts.get(key)
        if cached is None:
            if len(self._consts) > 16:
                self._consts.clear()
            t = torch.tensor(list(t_values), dtype=torch.int32).to(self.device)
            cond = torch.tensor([1.0 if m == COND_ONE else 0.0 for m in cond_modes], dtype=torch.float32).to(self.device)
            present = torch.tensor([0 if m == COND_NONE else 1 for m in cond_modes], dtype=torch.uint8).to(self.device)
            cached = self._consts[key] = (t, cond, present)
        return self.time_bias_general(cached[0], cached[1], cached[2], rows)

    def time_bias_general(self, t_i32, cond_f32, present_u8, rows):
        out = torch.empty(rows, self.tb_stride, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            check(self.lib.dt_unet_time_bias(self.h, ptr(t_i32), ptr(cond_f32), ptr(present_u8), rows, ptr(out),
                                             stream_ptr()), "dt_unet_time_bias")
        return out

    def forward(self, x, tb, n_pass, tb_div, tune=None):
        """eps[n_pass*B,C,H,W] for x[B,C,H,W]; tb rows as documented in dt_hip.h."""
        _require_cuda(x, "x")
        B, C, H, W = x.shape
        if C != self.channels:
            raise HipLibraryError(f"x has {C} channels, the model expects {self.channels}")
        return self._forward(x, tb, _Split(B, n_pass, 0, tb_div, False), tune)

    def forward_mixed(self, x, tb, b_single, tb_div, tune=None):
        """eps[2B - b_single, C, H, W] of a mixed batch (dt_unet_forward_mixed): images [0, b_single) take one pass,
        the others two; rows [pass 0 of all images | pass 1 of images b_single..]; row r uses tb[r // tb_div]."""
        _require_cuda(x, "x")
        return self._forward(x, tb, _Split(x.shape[0], 2, b_single, tb_div, True), tune)

    def _forward(self, x, tb, split, tune=None):
        """One forward of the batch ``split`` of x[B,C,H,W], through the entry the split names, under the shape's launch plan."""
        x = x.contiguous().float()
        B, C, H, W = x.shape
        rows = split.rows
        eps = torch.empty(rows, C, H, W, dtype=torch.float32, device=self.device)
        ws = self.workspace(rows, H, W)
        tail = (H, W, ptr(tb), split.tb_div, ptr(eps), ptr(ws), c_size_t(ws.numel()))

        def run():
            with torch.cuda.device(self.device):
                if split.mixed:
                    check(self.lib.dt_unet_forward_mixed(self.h, ptr(x), B, split.b_single, *tail, stream_ptr()), "dt_unet_forward_mixed")
                else:
                    check(self.lib.dt_unet_forward(self.h, ptr(x), B, split.n_pass, *tail, stream_ptr()), "dt_unet_forward")
        self.ensure_plan(rows, H, W, B, split.b_single, tune, run)
        run()
        return eps

    def block_features(self, x, tb, n_pass, tb_div, blocks=range(8)):
        """The outputs of the residual blocks ``blocks`` (indices into BLOCK_NAMES: enc1..enc4, bottleneck, dec3..dec1) for
        x [B, C, H, W], as ``PitchedFeatures`` over [n_pass * B, h, w, cp] views with the model's real channel counts: one
        forward on the layered kernels with the head launched separately, so that every block output is stored (small
        models that the fused kernel would serve included).  tb, n_pass and tb_div as in ``forward``.

        The views ALIAS the handle's workspace: they hold until the handle's next forward or sampler call of this shape on
        this stream; form the Grams (``device_cka_gram``) or copy (``.dense()``) before that.  The handle's head-fusion and
        fused switches and its launch plans are as they were afterwards: a later ``forward`` gives the bits it gave before."""
        _require_cuda(x, "x")
        blocks = [int(j) for j in blocks]
        if not blocks or any(not 0 <= j < _hip.N_BLOCKS for j in blocks):
            raise ValueError(f"blocks must name some of the {_hip.N_BLOCKS} residual blocks, got {blocks}")
        B, C, H, W = x.shape
        if C != self.channels:
            raise HipLibraryError(f"x has {C} channels, the model expects {self.channels}")
        split = _Split(B, n_pass, 0, tb_div, False)
        if self.shape(split.rows, H, W, B, 0) not in self._plans:
            self._forward(x, tb, split)          # the shape's launch plan is settled as any other caller settles it
        was = self._head_fusion
        self.set_head_fusion(False)              # the fused whole-forward kernel needs the fused head: this selects the layered path
        try:
            self._forward(x, tb, split)
        finally:
            self.set_head_fusion(was)
        real = [self.dims[0], self.dims[1], self.dims[2], self.dims[3], self.dims[3], self.dims[2], self.dims[1], self.dims[0]]
        return [PitchedFeatures(self.debug_activation(split.rows, H, W, j), real[j]) for j in blocks]

    def debug_activation(self, batch_total, H, W, which):
        """NHWC view [Bt,h,w,cp] of block ``which``'s output inside the workspace of the last forward (``which`` = 9, 10, 11: of
        the concat [upsampled | skip] that dec3, dec2, dec1 read)."""
        off, cp, oh, ow = c_size_t(), c_int(), c_int(), c_int()
        check(self.lib.dt_unet_debug_activation(self.h, batch_total, H, W, which, ctypes.byref(off), ctypes.byref(cp),
                                                ctypes.byref(oh), ctypes.byref(ow)), "dt_unet_debug_activation")
        ws = self.workspace(batch_total, H, W).view(torch.float32)
        n = batch_total * oh.value * ow.value * cp.value
        return ws[off.value: off.value + n].view(batch_total, oh.value, ow.value, cp.value)

    def _sample(self, rule, traj, H, W, tb, split, coef, has_noise, z, z_row, z_shift, w, w_scalar, mask=None, known=None,
                mask_row=None, known_row=None):
        """len(coef) reverse steps in place on traj[(n_steps+1), B, E] of the batch ``split``: the masked entry when a mask is
        given, else the entry the split names.  A shape that has no launch plan yet runs one forward first, which settles it."""
        n_steps = len(coef)
        B = traj.shape[1]
        assert traj.shape[0] == n_steps + 1 and traj.is_contiguous() and traj.dtype == torch.float32
        for name, t, row in (("mask", mask, mask_row), ("known", known, known_row)) if mask is not None else ():
            E = traj.shape[2]
            if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != E:
                raise HipLibraryError(f"sample_masked: {name} must be a contiguous float32 [rows, {E}] tensor, got {tuple(t.shape)} {t.dtype}")
            if row is None and t.shape[0] < B:
                raise HipLibraryError(f"sample_masked: {name} has {t.shape[0]} rows for {B} images and no row table")
            if row is not None and (row.dtype != torch.int32 or row.numel() != B or not row.is_cuda):
                raise HipLibraryError(f"sample_masked: {name}_row must be an int32 device tensor of {B} entries")
        coef_c = (c_float * (4 * n_steps))(*[float(v) for row in coef for v in (list(row) + [0.0] * 4)[:4]])
        noise_c = (c_int32 * n_steps)(*[int(bool(v)) for v in has_noise])
        shift_c = (c_int64 * n_steps)(*[int(v) for v in (z_shift if z_shift is not None else [0] * n_steps)])
        rows = split.rows
        ws = self.workspace(rows, H, W)
        if n_steps and self.shape(rows, H, W, B, split.b_single) not in self._plans:
            self._forward(traj[0].reshape(B, self.channels, H, W), tb[:rows // split.tb_div].contiguous(),
                          split._replace(n_pass=2) if split.mixed else split)
        noise = (coef_c, noise_c, ptr(z), ptr(z_row), shift_c, ptr(w))
        with torch.cuda.device(self.device):
            tail = (ptr(traj), ptr(ws), c_size_t(ws.numel()), stream_ptr())
            if mask is not None:
                check(self.lib.dt_sample_trajectory_masked(self.h, rule, B, split.n_pass, split.b_single, H, W, n_steps, ptr(tb), split.tb_div,
                                                           *noise, c_float(w_scalar), ptr(mask), ptr(mask_row), ptr(known), ptr(known_row),
                                                           *tail), "dt_sample_trajectory_masked")
            elif split.mixed:
                check(self.lib.dt_sample_trajectory_mixed(self.h, rule, B, split.b_single, H, W, n_steps, ptr(tb), split.tb_div, *noise, *tail),
                      "dt_sample_trajectory_mixed")
            else:
                check(self.lib.dt_sample_trajectory(self.h, rule, B, split.n_pass, H, W, n_steps, ptr(tb), *noise, c_float(w_scalar), *tail),
                      "dt_sample_trajectory")
        return traj

    def sample(self, rule, traj, H, W, tb, n_pass, coef, has_noise, z=None, z_row=None, z_shift=None, w=None,
               w_scalar=1.0):
        """Run len(coef) reverse steps in place on traj[(n_steps+1), B, E] (slot 0 = x_T)."""
        _require_cuda(traj, "traj")
        B = traj.shape[1]
        return self._sample(rule, traj, H, W, tb, _Split(B, n_pass, 0, B, False), coef, has_noise, z, z_row, z_shift, w, w_scalar)

    def sample_mixed(self, rule, traj, H, W, tb, tb_div, b_single, coef, has_noise, z, z_row, z_shift, w):
        """len(coef) reverse steps in place on traj[(n_steps+1), B, E] of a mixed batch (dt_sample_trajectory_mixed)."""
        _require_cuda(traj, "traj")
        return self._sample(rule, traj, H, W, tb, _Split(traj.shape[1], 2, b_single, tb_div, True), coef, has_noise, z, z_row, z_shift, w, 1.0)

    def sample_masked(self, rule, traj, H, W, tb, n_pass, coef, has_noise, mask, known, mask_row=None, known_row=None, z=None,
                      z_row=None, z_shift=None, w=None, w_scalar=1.0, b_single=0, tb_div=None):
        """``sample`` (``b_single`` > 0: ``sample_mixed``) with the known-region blend after every update
        (dt_sample_trajectory_masked): row b of traj keeps ``known[known_row[b]]`` where ``mask[mask_row[b]]`` is 0.  mask and
        known are fp32 device tensors [rows, E]; a row table that is None is the identity."""
        _require_cuda(traj, "traj"); _require_cuda(mask, "mask"); _require_cuda(known, "known")
        B = traj.shape[1]
        split = _Split(B, n_pass, b_single, B if tb_div is None else tb_div, bool(b_single))
        return self._sample(rule, traj, H, W, tb, split, coef, has_noise, z, z_row, z_shift, w, w_scalar, mask, known, mask_row, known_row)


def cfg_update_masked(rule, x, eps_u, eps_c, z, coef, has_noise, mask, known, mask_row=None, known_row=None, w=None,
                      w_scalar=1.0, z_row=None):
    """``cfg_update`` followed by the known-region blend ``m * x' + (1 - m) * known`` (dt_cfg_update_masked); mask and known
    are fp32 device tensors of rows of x[0].numel() elements, picked per image by the row tables (None: row b)."""
    lib = _hip.load()
    _require_cuda(x, "x"); _require_cuda(mask, "mask"); _require_cuda(known, "known")
    B, E = x.shape[0], x[0].numel()
    out = torch.empty_like(x)
    coef_c = (c_float * 4)(*(list(coef) + [0.0] * 4)[:4])
    with torch.cuda.device(x.device):
        check(lib.dt_cfg_update_masked(rule, ptr(x), ptr(eps_u), ptr(eps_c), ptr(z), ptr(z_row), coef_c, int(bool(has_noise)),
                                       ptr(w), c_float(w_scalar), ptr(out), B, E, stream_ptr(), ptr(mask), ptr(mask_row),
                                       ptr(known), ptr(known_row)), "dt_cfg_update_masked")
    return out


def edit_start(images, z, mask, B, img_row=None, z_row=None, mask_row=None, x_out=None):
    """(known [n_img, E], x [B, E]) of dt_edit_start: ``known = 2 * images - 1`` and the start states
    ``x[b] = m * z[z_row[b]] + (1 - m) * known[img_row[b]]`` with ``m = mask[mask_row[b]]``.  images in [0, 1], z and mask
    are fp32 device tensors of rows of E elements; ``x_out`` (e.g. slot 0 of a trajectory buffer) is written when given."""
    lib = _hip.load()
    _require_cuda(images, "images"); _require_cuda(z, "z"); _require_cuda(mask, "mask")
    images, z, mask = (t.reshape(t.shape[0], -1).contiguous().float() for t in (images, z, mask))
    n_img, E = images.shape
    if z.shape[1] != E or mask.shape[1] != E:
        raise HipLibraryError(f"edit_start: rows of {E} (images), {z.shape[1]} (z) and {mask.shape[1]} (mask) elements")
    for name, t, row in (("images", images, img_row), ("z", z, z_row), ("mask", mask, mask_row)):
        if row is None and t.shape[0] < B:
            raise HipLibraryError(f"edit_start: {name} has {t.shape[0]} rows for {B} cells and no row table")
    known = torch.empty_like(images)
    x = torch.empty(B, E, dtype=torch.float32, device=images.device) if x_out is None else x_out
    with torch.cuda.device(images.device):
        check(lib.dt_edit_start(ptr(images), ptr(img_row), n_img, ptr(z), ptr(z_row), ptr(mask), ptr(mask_row), ptr(known),
                                ptr(x), B, E, stream_ptr()), "dt_edit_start")
    return known, x


def device_masked_pair_stats(X, Y, mask, known, mask_row=None, known_row=None):
    """float64 [B, n, 4] = {sum m (x-y)^2, sum m (x-k)^2, sum m (y-k)^2, sum (1-m) (x-y)^2} per state of X, Y [n, B, E]
    (dt_masked_pair_stats; E % 4 == 0), m and k the mask / known rows of image b."""
    lib = _hip.load()
    _require_cuda(X, "X"); _require_cuda(Y, "Y"); _require_cuda(mask, "mask"); _require_cuda(known, "known")
    X, Y = X.contiguous(), Y.contiguous()
    n, B, E = X.shape
    if tuple(Y.shape) != (n, B, E) or mask.shape[-1] != E or known.shape[-1] != E:
        raise HipLibraryError(f"device_masked_pair_stats: X {tuple(X.shape)}, Y {tuple(Y.shape)}, mask {tuple(mask.shape)}, known {tuple(known.shape)}")
    out = torch.empty(B, n, 4, dtype=torch.float64, device=X.device)
    with torch.cuda.device(X.device):
        check(lib.dt_masked_pair_stats(ptr(X), ptr(Y), n, B, E, ptr(mask.contiguous()), ptr(mask_row), ptr(known.contiguous()),
                                       ptr(known_row), ptr(out), stream_ptr()), "dt_masked_pair_stats")
    return out


def cfg_update(rule, x, eps_u, eps_c, z, coef, has_noise, w=None, w_scalar=1.0, z_row=None):
    """One fused CFG-mix + update step (dt_cfg_update); returns the new x."""
    lib = _hip.load()
    _require_cuda(x, "x")
    B, E = x.shape[0], x[0].numel()
    out = torch.empty_like(x)
    coef_c = (c_float * 4)(*(list(coef) + [0.0] * 4)[:4])
    with torch.cuda.device(x.device):
        check(lib.dt_cfg_update(rule, ptr(x), ptr(eps_u), ptr(eps_c), ptr(z), ptr(z_row), coef_c, int(bool(has_noise)),
                                ptr(w), c_float(w_scalar), ptr(out), B, E, stream_ptr()), "dt_cfg_update")
    return out


# ---------------------------------------------------------------------- module-level forward
def time_bias_rows(handle, B, t, cond=None):
    """(tb, tb_div) of a forward of B images for ``model(x, t, cond)``'s arguments: t [B], [1] or a scalar, cond [B, 1], [1, 1]
    or None, broadcast as the reference's forward does; one row shared by the batch when both are single."""
    t = torch.as_tensor(t)
    t = t.reshape(1) if t.dim() == 0 else (t.reshape(t.shape[0], -1)[:, 0] if t.dim() > 1 else t)
    rows = t.shape[0]
    c = None
    if cond is not None:
        c = cond.reshape(cond.shape[0], -1)[:, 0].float()
        rows = max(rows, c.shape[0])
    if rows not in (1, B):
        raise RuntimeError(f"time/condition rows ({rows}) cannot broadcast onto batch {B}")
    t_i = t.to(device=handle.device, dtype=torch.int32).expand(rows).contiguous()
    c_f = c.to(handle.device).expand(rows).contiguous() if c is not None else None
    return handle.time_bias_general(t_i, c_f, None, rows), (B if rows == 1 else 1)


def unet_forward_module(module, x, t, cond=None):
    """General ``model(x, t, cond)`` (reference models.py:159-224): per-row t / cond with broadcasting."""
    _require_cuda(x, "x")
    h = UNetHandle.for_module(module)
    tb, tb_div = time_bias_rows(h, x.shape[0], t, cond)
    return h.forward(x, tb, 1, tb_div)


# ---------------------------------------------------------------------- metrics
def _pad_quads(t):
    """t [n, B, E] with the coordinate axis zero-padded to a multiple of 4: dt_traj_metrics and dt_pair_stats load float4
    quads and take E % 4 == 0 only.  Padding BOTH operands with zeros adds exactly 0 to every one of their sums (endpoint
    rows included); the Wasserstein and resampled-distance kernels take any E and get the unpadded tensors."""
    E = t.shape[-1]
    return t if E % 4 == 0 else torch.nn.functional.pad(t, (0, -E % 4)).contiguous()


def device_metric_sums(X, Y):
    """float64 [B, n_max, 4] sums of dt_traj_metrics for trajectories X[nT,B,E], Y[nS,B,E] on device (any E)."""
    lib = _hip.load()
    _require_cuda(X, "teacher trajectory"); _require_cuda(Y, "student trajectory")
    X, Y = _pad_quads(X), _pad_quads(Y)
    nT, B, E = X.shape
    nS = Y.shape[0]
    out = torch.empty(B, max(nT, nS), 4, dtype=torch.float64, device=X.device)
    with torch.cuda.device(X.device):
        check(lib.dt_traj_metrics(ptr(X), ptr(Y), nT, nS, B, E, ptr(out), stream_ptr()), "dt_traj_metrics")
    return out


def device_wasserstein(X, Y, index=None, index_row=None):
    """float64 [B, n] per-step W1 over the first n = min(len) states; index int32 [tables, n, n_idx] or
    None (all coordinates); index_row int32 [B] picks each pair's table (None: table 0)."""
    lib = _hip.load()
    n = min(X.shape[0], Y.shape[0])
    _, B, E = X.shape
    out = torch.empty(B, n, dtype=torch.float64, device=X.device)
    n_idx = 0 if index is None else index.shape[-1]
    with torch.cuda.device(X.device):
        check(lib.dt_traj_wasserstein(ptr(X), ptr(Y), n, B, E, ptr(index), ptr(index_row), n_idx, ptr(out), stream_ptr()),
              "dt_traj_wasserstein")
    return out


def device_pair_metrics(X, Y, index=None, index_row=None):
    """(sums float64 [B, n_max, 4], w1 float64 [B, min(n)]) of ``device_metric_sums`` and ``device_wasserstein`` -- in ONE
    launch (dt_traj_pair_metrics: each state read from HBM once, register / cross-lane sort) when the trajectories have equal
    lengths and the Wasserstein term uses all E <= 4096 coordinates, otherwise through the two separate kernels."""
    lib = _hip.load()
    _require_cuda(X, "teacher trajectory"); _require_cuda(Y, "student trajectory")
    n, B, E = X.shape
    if index is not None or Y.shape[0] != n or E > 4096 or E % 4 or B > 65535:
        return device_metric_sums(X, Y), device_wasserstein(X, Y, index, index_row)
    sums = torch.empty(B, n, 4, dtype=torch.float64, device=X.device)
    w1 = torch.empty(B, n, dtype=torch.float64, device=X.device)
    with torch.cuda.device(X.device):
        check(lib.dt_traj_pair_metrics(ptr(X), ptr(Y), n, B, E, ptr(sums), ptr(w1), stream_ptr()), "dt_traj_pair_metrics")
    return sums, w1


def device_pair_stats(X, Y):
    """float64 [B, n, 5] = {sum (x-y)^2, sum |x-y|, sum xy, sum x^2, sum y^2} for X, Y [n, B, E] (dt_pair_stats, any E)."""
    lib = _hip.load()
    _require_cuda(X, "X"); _require_cuda(Y, "Y")
    X, Y = _pad_quads(X), _pad_quads(Y)
    n, B, E = X.shape
    out = torch.empty(B, n, 5, dtype=torch.float64, device=X.device)
    with torch.cuda.device(X.device):
        check(lib.dt_pair_stats(ptr(X), ptr(Y), n, B, E, ptr(out), stream_ptr()), "dt_pair_stats")
    return out


def q_sample(x0, z, coef):
    """fp32 [G, B, ...] = coef[g, 0] * x0 + coef[g, 1] * z[g] for x0 [B, ...], z [G, B, ...] and coef [G, 2] (dt_q_sample:
    the forward noising of the noise-prediction analysis, bit-identical to the torch expression)."""
    lib = _hip.load()
    _require_cuda(x0, "x0"); _require_cuda(z, "z"); _require_cuda(coef, "coef")
    x0, z, coef = x0.contiguous().float(), z.contiguous().float(), coef.contiguous().float()
    G, B = z.shape[0], x0.shape[0]
    E = x0[0].numel()
    if tuple(z.shape[1:]) != tuple(x0.shape) or tuple(coef.shape) != (G, 2):
        raise HipLibraryError(f"q_sample: z {tuple(z.shape)} / coef {tuple(coef.shape)} do not match x0 {tuple(x0.shape)}")
    out = torch.empty_like(z)
    with torch.cuda.device(x0.device):
        check(lib.dt_q_sample(ptr(x0), ptr(z), ptr(coef), G, B, E, ptr(out), stream_ptr()), "dt_q_sample")
    return out


def device_sample_mean(traj):
    """fp32 [n, E]: mean over the B samples of traj [n, B, E] (dt_traj_sample_mean)."""
    lib = _hip.load()
    _require_cuda(traj, "traj")
    n, B, E = traj.shape
    out = torch.empty(n, E, dtype=torch.float32, device=traj.device)
    with torch.cuda.device(traj.device):
        check(lib.dt_traj_sample_mean(ptr(traj), n, B, E, ptr(out), stream_ptr()), "dt_traj_sample_mean")
    return out


# ---------------------------------------------------------------------- sampler noise on the device (include/dt_hip_rng.h)
RNG_STATE_WORDS = 624           # DT_RNG_STATE_WORDS
RNG_MIN_ELEMENTS = 16           # below it torch.randn takes a double-precision scalar path that the library does not provide


def noise_mode(noise=None):
    """"host" or "device": ``noise`` if given, else ``$DT_NOISE``, else "host".  "host" draws sampler noise with the torch
    CPU generator and uploads it; "device" makes the same numbers on the device (``device_randn``)."""
    mode = noise if noise is not None else (os.environ.get("DT_NOISE") or "host")
    if mode not in ("host", "device"):
        raise ValueError(f"noise (or DT_NOISE) must be 'host' or 'device', got {mode!r}")
    return mode


class HostGenerator:
    """The global torch CPU generator as the library's (state words, position): ``words`` uint32 [624], ``pos`` in 0..624
    (624: the block is used up, or the generator is fresh from ``manual_seed``), read from the 5056 bytes of
    ``torch.get_rng_state()`` (seed 8 bytes, left int32, seeded 4 bytes, next 8 bytes, 624 words as uint64, then the
    normal-sample cache).  ``write`` puts a walk's end back: seed, seeded flag and the cache stay as they were read."""
    STATE_BYTES = 5056

    def __init__(self, raw=None):
        raw = torch.get_rng_state() if raw is None else raw
        b = np.array(raw.numpy() if isinstance(raw, torch.Tensor) else raw, dtype=np.uint8)
        if b.shape != (self.STATE_BYTES,):
            raise ValueError(f"a torch CPU generator state has {self.STATE_BYTES} bytes, got {b.shape}")
        self.raw = b
        left, nxt = int(b[8:12].view(np.int32)[0]), int(b[16:24].view(np.uint64)[0])
        self.words = b[24:24 + 8 * RNG_STATE_WORDS].view(np.uint64).astype(np.uint32)
        self.pos = RNG_STATE_WORDS if left == 1 else nxt
        if not 0 <= self.pos <= RNG_STATE_WORDS:
            raise ValueError(f"generator state with next = {nxt}")

    def state_bytes(self, words, pos):
        """The 5056 bytes of this generator moved to (``words``, ``pos``): next = pos and left = 625 - pos, which is how the
        generator leaves them once it has produced a word."""
        words, pos = np.asarray(words).reshape(-1).view(np.uint32), int(pos)
        if words.shape != (RNG_STATE_WORDS,) or not 0 <= pos <= RNG_STATE_WORDS:
            raise ValueError("an mt19937 state is 624 words and a position in 0..624")
        b = self.raw.copy()
        b[8:12] = np.array([RNG_STATE_WORDS + 1 - pos], np.int32).view(np.uint8)
        b[16:24] = np.array([pos], np.uint64).view(np.uint8)
        b[24:24 + 8 * RNG_STATE_WORDS] = words.astype(np.uint64).view(np.uint8)
        return b

    def write(self, words, pos):
        """``torch.set_rng_state`` of ``state_bytes(words, pos)``; ``words`` / ``pos`` may be the device tensors an entry
        returned (one stream)."""
        if isinstance(words, torch.Tensor):
            words = words.detach().cpu().contiguous().numpy()
        if isinstance(pos, torch.Tensor):
            pos = int(pos.reshape(-1)[0])
        torch.set_rng_state(torch.from_numpy(self.state_bytes(words, pos)))


def _rng_start(seeds, state, device):
    """(seeds, state words, positions) device tensors (None where unused), S and the device of a call's streams."""
    if (seeds is None) == (state is None):
        raise ValueError("give either seeds= or state=")
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise HipLibraryError(f"the device RNG runs on the GPU only, got device {device}")
    if seeds is not None:
        if isinstance(seeds, torch.Tensor):
            vals = [int(v) for v in seeds.reshape(-1).tolist()]
        else:
            vals = [int(v) for v in (seeds if isinstance(seeds, (list, tuple, range, np.ndarray)) else [seeds])]
        if not vals:
            raise ValueError("seeds is empty")
        # torch.manual_seed keys the mt19937 with the seed mod 2**32
        return torch.tensor([v % 2 ** 32 for v in vals], dtype=torch.int64, device=device), None, None, len(vals), device
    words, pos = (state.words, state.pos) if isinstance(state, HostGenerator) else state
    if isinstance(words, torch.Tensor):
        words = words.to(device).contiguous()
        if words.dtype != torch.int32:
            raise ValueError("state words as a tensor are int32 (the bits of the uint32 words)")
    else:
        words = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(device)
    words = words.reshape(-1, RNG_STATE_WORDS)
    S = words.shape[0]
    if isinstance(pos, torch.Tensor):
        pos = pos.to(device=device, dtype=torch.int32).reshape(-1).contiguous()
    else:
        plist = [int(v) for v in np.asarray(pos).reshape(-1)]
        if any(not 0 <= v <= RNG_STATE_WORDS for v in plist):
            raise ValueError("a position is in 0..624")
        pos = torch.tensor(plist, dtype=torch.int32, device=device)
    if pos.numel() != S:
        raise ValueError(f"{S} states but {pos.numel()} positions")
    return None, words, pos, S, device


def device_mt19937_words(seeds=None, state=None, n=0, skip=0, out=None, device=None, return_state=False):
    """int32 [S, n]: the bits of ``n`` tempered mt19937 words of each stream after skipping ``skip`` (dt_rng_mt19937_words).
    Streams start from ``seeds`` (an int or a sequence; what ``torch.manual_seed`` would key) or from ``state``, a
    ``HostGenerator`` or ``(words [S, 624], pos [S])``.  ``return_state``: also ``(words int32 [S, 624], pos int32 [S])`` on the
    device where the walks end."""
    lib = _hip.load()
    seeds_t, st_t, pos_t, S, device = _rng_start(seeds, state, device)
    n, skip = int(n), int(skip)
    if out is None:
        out = torch.empty(S, max(n, 0), dtype=torch.int32, device=device)
    _require_cuda(out, "out")
    if out.dtype != torch.int32 or not out.is_contiguous() or out.dim() != 2 or out.shape[0] != S or out.shape[1] < n:
        raise ValueError(f"out must be a contiguous int32 [S, >= n] tensor, got {tuple(out.shape)} {out.dtype}")
    end = (torch.empty(S, RNG_STATE_WORDS, dtype=torch.int32, device=device),
           torch.empty(S, dtype=torch.int32, device=device)) if return_state else (None, None)
    with torch.cuda.device(device):
        check(lib.dt_rng_mt19937_words(ptr(seeds_t), ptr(st_t), ptr(pos_t), S, skip, n, ptr(out), out.shape[1], ptr(end[0]),
                                       ptr(end[1]), stream_ptr()), "dt_rng_mt19937_words")
    return (out, end) if return_state else out


def device_randn(seeds=None, state=None, draws=1, E=None, out=None, strides=None, skip=0, device=None, return_state=False,
                 workspace=None):
    """The draws ``torch.randn(E)`` would give on the host, made on the device (dt_rng_randn), bit for bit.

    Every stream (``seeds`` or ``state`` as for ``device_mt19937_words``) gives ``draws`` consecutive draws of ``E >= 16``
    fp32 elements after skipping ``skip`` words.  ``draws`` is a count, or ``(A, B)``: draw ``a * B + b`` of stream ``s`` is
    written at ``out.view(-1)[s * strides[0] + a * strides[1] + b * strides[2] :][:E]`` and nothing else of ``out`` is
    touched; the default is a new ``[S, A * B, E]`` tensor.  With ``state`` a ``HostGenerator`` the global CPU generator
    is afterwards where the same draws on the host would have left it.  ``return_state``: also the end ``(words, pos)``.
    ``workspace``: a uint8 device tensor of any size from ``dt_rng_workspace_bytes(S, 1, E)`` up (default: the
    library's bounded suggestion)."""
    lib = _hip.load()
    if E is None:
        raise ValueError("E, the elements per draw, is required")
    E, skip = int(E), int(skip)
    if E < RNG_MIN_ELEMENTS:
        raise HipLibraryError(f"device_randn draws at least {RNG_MIN_ELEMENTS} elements per draw, got E = {E}: below that "
                              "torch.randn takes a double-precision scalar path that the library does not provide (DT_E_ARG)")
    seeds_t, st_t, pos_t, S, device = _rng_start(seeds, state, device)
    A, B = (int(draws[0]), int(draws[1])) if isinstance(draws, (tuple, list)) else (int(draws), 1)
    n_draws = max(A, 0) * max(B, 0)
    if out is None:
        if strides is not None:
            raise ValueError("strides need out")
        out = torch.empty(S, n_draws, max(E, 0), dtype=torch.float32, device=device)
        strides = (n_draws * E, B * E, E)
    elif strides is None:
        strides = (n_draws * E, B * E, E)
    _require_cuda(out, "out")
    ss, sa, sb = (int(v) for v in strides)
    if out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor")
    if min(ss, sa, sb) < 0:
        raise ValueError("strides are non-negative counts of floats")
    if n_draws > 0 and E > 0 and (S - 1) * ss + (A - 1) * sa + (B - 1) * sb + E > out.numel():
        raise ValueError(f"draws {(S, A, B)} of {E} elements with strides {(ss, sa, sb)} do not fit out ({out.numel()} floats)")
    host = state if isinstance(state, HostGenerator) else None
    want_state = return_state or (host is not None and n_draws > 0)
    end = (torch.empty(S, RNG_STATE_WORDS, dtype=torch.int32, device=device),
           torch.empty(S, dtype=torch.int32, device=device)) if want_state else (None, None)
    if workspace is None:
        need = lib.dt_rng_workspace_bytes(S, n_draws, E)
        workspace = torch.empty(max(need, 4), dtype=torch.uint8, device=device)
    _require_cuda(workspace, "workspace")
    with torch.cuda.device(device):
        check(lib.dt_rng_randn(ptr(seeds_t), ptr(st_t), ptr(pos_t), S, skip, A, B, E, ptr(out), ss, sa, sb, ptr(end[0]),
                               ptr(end[1]), ptr(workspace), workspace.numel(), stream_ptr()), "dt_rng_randn")
    if host is not None and n_draws > 0:
        host.write(end[0][0], end[1][0])
    return (out, end) if return_state else out


# ---------------------------------------------------------------------- fp64 dense stages (csrc/dt_dense64.h)
def _f32_rows(t, name, layouts):
    """t, a float32 torch tensor of 2 or 3 dims (``layouts`` names them in the error); shape errors are ValueErrors."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if t.dim() not in (2, 3):
        raise ValueError(f"{name} must be {layouts}, got shape {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    return t


def _aligned_rows(t):
    """t as the kernels read its rows (float4 loads): unit column stride, a 16-byte aligned base and every other stride a
    multiple of 4 elements; a contiguous copy where it is not so"""
    if t.stride(-1) != 1 or t.data_ptr() % 16 or any(s % 4 for s in t.stride()[:-1]):
        return t.contiguous()
    return t


def _stage_events(events):
    """the ``void *const *events`` argument of dt_pca_fit / dt_fid_distance: None, or the HIP events of the
    torch.cuda.Event list (torch creates the HIP event at its first record)"""
    if events is None:
        return None
    for e in events:
        e.record()
    return (c_void_p * len(events))(*[e._as_parameter_.value for e in events])


# ---------------------------------------------------------------------- PCA (include/dt_hip_pca.h)
PCA_MAX_K = 16


def _pca_rows(t, name):
    """[n, P, E] view of a step-major tensor (a 2-D [n, E] tensor is one problem)"""
    t = _f32_rows(t, name, "[n, E] or step-major [n, P, E]")
    return t.unsqueeze(1) if t.dim() == 2 else t


def _pca_pad(t, E4):
    """t [n, P, E] as the kernel reads it: rows 16-byte aligned, E zero-padded to E4 (a PCA is blind to zero columns)."""
    E = t.shape[-1]
    return _aligned_rows(t) if E == E4 else torch.nn.functional.pad(t, (0, E4 - E)).contiguous()


def _pca_check(a, b, k):
    a = _pca_rows(a, "a")
    b = None if b is None else _pca_rows(b, "b")
    n_a, P, E = a.shape
    n_b = 0 if b is None else b.shape[0]
    if b is not None and tuple(b.shape[1:]) != (P, E):
        raise ValueError(f"b {tuple(b.shape)} does not match a {tuple(a.shape)}: every row needs the same length and the "
                         "same number of problems")
    n = n_a + n_b
    if n < 2 or n_a < 1:
        raise ValueError(f"a PCA needs n >= 2 rows (a first), got n_a={n_a}, n_b={n_b}")
    if not 1 <= P <= 65535 or E < 1:
        raise ValueError(f"unsupported shape: P={P}, E={E}")
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= min(PCA_MAX_K, n - 1, E):
        raise ValueError(f"n_components={k!r} must be an int in [1, min({PCA_MAX_K}, n - 1, E)] = [1, "
                         f"{min(PCA_MAX_K, n - 1, E)}]")
    return a, b, int(k)


def device_pca(a, k, b=None, events=None):
    """Exact PCA (sklearn ``PCA(k, svd_solver="full")`` on the float64 copy) of every problem p of the step-major device
    tensors a [n_a, P, E] and b [n_b, P, E] (rows a[:, p] then b[:, p]; a 2-D [n, E] tensor is one problem), in place
    when the rows are 16-byte aligned and E % 4 == 0.  Returns device tensors {mean [P, E] fp32, components [P, k, E] fp32,
    scores [P, n, k] fp32, singular_values / explained_variance / explained_variance_ratio [P, k] fp64, status [P] int32}
    (status: 0 ok, 1 non-finite input, 2 zero total variance).  ``events``: None or 4 torch.cuda.Event(enable_timing=True)
    recorded at the stage boundaries (dt_pca_fit)."""
    a, b, k = _pca_check(a, b, k)
    _require_cuda(a, "a")
    if b is not None:
        _require_cuda(b, "b")
    lib = _hip.load()
    n_a, P, E = a.shape
    n_b = 0 if b is None else b.shape[0]
    n, E4 = n_a + n_b, E + (-E % 4)
    a = _pca_pad(a, E4)
    b = None if b is None else _pca_pad(b, E4)
    dev = a.device
    f32 = dict(dtype=torch.float32, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    out = {"mean": torch.empty(P, E4, **f32), "components": torch.empty(P, k, E4, **f32),
           "scores": torch.empty(P, n, k, **f32), "singular_values": torch.empty(P, k, **f64),
           "explained_variance": torch.empty(P, k, **f64), "explained_variance_ratio": torch.empty(P, k, **f64),
           "status": torch.empty(P, dtype=torch.int32, device=dev)}
    ws_bytes = lib.dt_pca_workspace_bytes(P, n, E4, k)
    if ws_bytes == 0:
        raise ValueError(f"dt_pca_workspace_bytes rejects P={P}, n={n}, E={E4}, k={k}")
    if events is not None and len(events) != 4:
        raise ValueError("events must be 4 torch.cuda.Event")
    ev = _stage_events(events)
    with torch.cuda.device(dev):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        bs = (0, 0) if b is None else (b.stride(1), b.stride(0))
        check(lib.dt_pca_fit(ptr(a), n_a, a.stride(1), a.stride(0), ptr(b), n_b, bs[0], bs[1], P, E4, k,
                             ptr(out["mean"]), ptr(out["components"]), ptr(out["scores"]), ptr(out["singular_values"]),
                             ptr(out["explained_variance"]), ptr(out["explained_variance_ratio"]), ptr(out["status"]),
                             ptr(ws), ws_bytes, ev, stream_ptr()), "dt_pca_fit")
    if E4 != E:
        out["mean"], out["components"] = out["mean"][:, :E], out["components"][:, :, :E]
    return out


def device_pca_project(a, mean, components, b=None):
    """fp32 scores [P, n, k] = (row - mean) . components^T (fp64 sums, dt_pca_project) for the rows of a [n_a, P, E] and
    b [n_b, P, E] (as in ``device_pca``); mean [E] / components [k, E] are one basis for every problem, [P, E] /
    [P, k, E] one per problem."""
    a = _pca_rows(a, "a")
    b = None if b is None else _pca_rows(b, "b")
    n_a, P, E = a.shape
    if b is not None and tuple(b.shape[1:]) != (P, E):
        raise ValueError(f"b {tuple(b.shape)} does not match a {tuple(a.shape)}")
    for t, name in ((mean, "mean"), (components, "components")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 tensor")
    shared = components.dim() == 2
    if shared and (tuple(mean.shape) != (E,) or components.shape[1] != E):
        raise ValueError(f"mean {tuple(mean.shape)} / components {tuple(components.shape)} do not match E={E}")
    if not shared and (components.dim() != 3 or tuple(mean.shape) != (P, E) or components.shape[0] != P
                       or components.shape[2] != E):
        raise ValueError(f"mean {tuple(mean.shape)} / components {tuple(components.shape)} do not match P={P}, E={E}")
    k = components.shape[-2]
    if not 1 <= k <= PCA_MAX_K or not 1 <= P <= 65535:
        raise ValueError(f"unsupported k={k} or P={P}")
    for t, name in ((a, "a"), (b, "b"), (mean, "mean"), (components, "components")):
        if t is not None:
            _require_cuda(t, name)
    lib = _hip.load()
    E4 = E + (-E % 4)
    a = _pca_pad(a, E4)
    b = None if b is None else _pca_pad(b, E4)
    mean = torch.nn.functional.pad(mean, (0, E4 - E)).contiguous()
    components = torch.nn.functional.pad(components, (0, E4 - E)).contiguous()
    n_b = 0 if b is None else b.shape[0]
    out = torch.empty(P, n_a + n_b, k, dtype=torch.float32, device=a.device)
    bs = (0, 0) if b is None else (b.stride(1), b.stride(0))
    with torch.cuda.device(a.device):
        check(lib.dt_pca_project(ptr(a), n_a, a.stride(1), a.stride(0), ptr(b), n_b, bs[0], bs[1], P, E4, k,
                                 ptr(mean), 0 if shared else E4, ptr(components), 0 if shared else k * E4, ptr(out),
                                 stream_ptr()), "dt_pca_project")
    return out


# ---------------------------------------------------------------------- t-SNE (include/dt_hip_tsne.h)
TSNE_MAX_N = 512


def tsne_state_doubles(n):
    """doubles of descent state per problem: y, update, gains [n, 2] each, then ctl (DT_TSNE_STATE_DOUBLES)"""
    return 6 * n + 4


def tsne_state_views(state, n):
    """{y, update, gains [P, n, 2], ctl [P, 4] = (best_error, best_iter, iterations done, stop reason)}: views of a
    ``device_tsne`` state tensor [P, 6 n + 4]"""
    P = state.shape[0]
    return {"y": state[:, :2 * n].view(P, n, 2), "update": state[:, 2 * n:4 * n].view(P, n, 2),
            "gains": state[:, 4 * n:6 * n].view(P, n, 2), "ctl": state[:, 6 * n:]}


def _real(x, name, low=None, strict=True):
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not math.isfinite(x):
        raise ValueError(f"{name}={x!r} must be a finite number")
    if low is not None and (x <= low if strict else x < low):
        raise ValueError(f"{name}={x!r} must be {'>' if strict else '>='} {low}")
    return float(x)


def _count(x, name, low=0):
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < low:
        raise ValueError(f"{name}={x!r} must be an int >= {low}")
    return int(x)


def _tsne_check(a, b, perplexity, init, max_iter, it_begin, state, affinities, early_exaggeration, learning_rate,
                n_iter_without_progress, min_grad_norm, exaggeration_iters, momentum, min_gain, n_iter_check):
    """every argument error of ``device_tsne`` as a ValueError, before any device work; returns the rows, the shape and a
    filled _hip.TsneParams"""
    a = _pca_rows(a, "a")
    b = None if b is None else _pca_rows(b, "b")
    n_a, P, E = a.shape
    n_b = 0 if b is None else b.shape[0]
    if b is not None and tuple(b.shape[1:]) != (P, E):
        raise ValueError(f"b {tuple(b.shape)} does not match a {tuple(a.shape)}: every row needs the same length and the "
                         "same number of problems")
    n = n_a + n_b
    if not 4 <= n <= TSNE_MAX_N or n_a < 1:
        raise ValueError(f"t-SNE needs 4 <= n <= {TSNE_MAX_N} rows (a first), got n_a={n_a}, n_b={n_b}")
    if not 1 <= P <= 65535 or E < 1:
        raise ValueError(f"unsupported shape: P={P}, E={E}")
    perplexity = _real(perplexity, "perplexity", 0.0)
    if perplexity >= n:
        raise ValueError(f"perplexity={perplexity} must be less than n={n}")
    it_begin, max_iter = _count(it_begin, "it_begin"), _count(max_iter, "max_iter")
    if max_iter < it_begin:
        raise ValueError(f"max_iter={max_iter} is below it_begin={it_begin}")
    if (init is None) == (state is None):
        raise ValueError("give exactly one of init (a fresh run) and state (a resumed one)")
    if init is not None:
        if isinstance(init, np.ndarray):
            init = torch.from_numpy(np.array(init))
        if not isinstance(init, torch.Tensor) or tuple(init.shape) not in ((n, 2), (P, n, 2)):
            raise ValueError(f"init must be an array or tensor [n, 2] or [P, n, 2] = [{P}, {n}, 2], got "
                             f"{tuple(init.shape) if hasattr(init, 'shape') else type(init).__name__}")
        if not init.dtype.is_floating_point:
            raise ValueError(f"init must be floating point, got {init.dtype}")
    else:
        if (not isinstance(state, torch.Tensor) or state.dtype != torch.float64
                or tuple(state.shape) != (P, tsne_state_doubles(n))):
            raise ValueError(f"state must be a float64 tensor [{P}, {tsne_state_doubles(n)}]")
    if affinities is not None and (not isinstance(affinities, torch.Tensor) or affinities.dtype != torch.float64
                                   or tuple(affinities.shape) != (P, n, n)):
        raise ValueError(f"affinities must be a float64 tensor [{P}, {n}, {n}]")
    prm = _hip.TsneParams()
    prm.early_exaggeration = _real(early_exaggeration, "early_exaggeration", 0.0)
    if isinstance(learning_rate, str):
        if learning_rate != "auto":
            raise ValueError(f"learning_rate={learning_rate!r} must be 'auto' or a positive number")
        prm.learning_rate = max(n / prm.early_exaggeration / 4.0, 50.0)
    else:
        prm.learning_rate = _real(learning_rate, "learning_rate", 0.0)
    if not isinstance(momentum, (tuple, list)) or len(momentum) != 2:
        raise ValueError(f"momentum={momentum!r} must be a pair")
    prm.momentum[0], prm.momentum[1] = _real(momentum[0], "momentum[0]"), _real(momentum[1], "momentum[1]")
    prm.min_gain = _real(min_gain, "min_gain", 0.0, strict=False)
    if isinstance(min_grad_norm, bool) or not isinstance(min_grad_norm, (int, float, np.integer, np.floating)) \
            or not min_grad_norm >= 0:
        raise ValueError(f"min_grad_norm={min_grad_norm!r} must be a number >= 0")
    prm.min_grad_norm = float(min_grad_norm)
    prm.exaggeration_iters = _count(exaggeration_iters, "exaggeration_iters")
    prm.n_iter_check = _count(n_iter_check, "n_iter_check", 1)
    if isinstance(n_iter_without_progress, (tuple, list)):
        if len(n_iter_without_progress) != 2:
            raise ValueError(f"n_iter_without_progress={n_iter_without_progress!r} must be an int or a pair")
        pair = n_iter_without_progress
    else:
        pair = (prm.exaggeration_iters, n_iter_without_progress)       # sklearn: the exaggerated stage allows its own length
    prm.n_iter_without_progress[0] = _count(pair[0], "n_iter_without_progress[0]")
    prm.n_iter_without_progress[1] = _count(pair[1], "n_iter_without_progress")
    return a, b, perplexity, init, prm


def device_tsne(a, b=None, perplexity=30.0, init=None, max_iter=1000, early_exaggeration=12.0, learning_rate="auto",
                n_iter_without_progress=300, min_grad_norm=1e-7, exaggeration_iters=250, momentum=(0.5, 0.8),
                min_gain=0.01, n_iter_check=50, it_begin=0, state=None, affinities=None, return_affinities=False):
    """Exact t-SNE (sklearn ``TSNE(method="exact")``, 2 components) of every problem p of the step-major device tensors
    a [n_a, P, E] and b [n_b, P, E] (rows a[:, p] then b[:, p]; a 2-D [n, E] tensor is one problem; 4 <= n <= 512), in
    place when the rows are 16-byte aligned and E % 4 == 0: dt_tsne_affinities, then iterations [it_begin, max_iter) of
    dt_tsne_descend in one launch.

    A fresh run takes ``init`` ([n, 2] for every problem, or [P, n, 2]); a resumed one takes the ``state`` an earlier call
    returned and its ``it_begin``; the state given is not changed.  ``affinities`` [P, n, n] fp64 from an earlier call
    skips their computation.  ``n_iter_without_progress`` is sklearn's argument (the exaggerated stage then allows
    ``exaggeration_iters``, as sklearn does) or a pair.  Returns device tensors {embedding [P, n, 2] fp32, kl_divergence
    [P] fp64 (of the returned embedding), n_iter [P] int32 (iterations done), status [P] int32 (0 ok, 1 non-finite input:
    embedding and KL are NaN), state [P, 6 n + 4] fp64 (``tsne_state_views``)} and, with ``return_affinities``,
    affinities [P, n, n] fp64."""
    a, b, perplexity, init, prm = _tsne_check(a, b, perplexity, init, max_iter, it_begin, state, affinities,
                                              early_exaggeration, learning_rate, n_iter_without_progress, min_grad_norm,
                                              exaggeration_iters, momentum, min_gain, n_iter_check)
    _require_cuda(a, "a")
    if b is not None:
        _require_cuda(b, "b")
    lib = _hip.load()
    n_a, P, E = a.shape
    n_b = 0 if b is None else b.shape[0]
    n, E4 = n_a + n_b, E + (-E % 4)
    dev = a.device
    f64 = dict(dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        if affinities is None:
            a = _pca_pad(a, E4)                              # squared distances are blind to zero columns
            b = None if b is None else _pca_pad(b, E4)
            ws_bytes = lib.dt_tsne_workspace_bytes(P, n, E4)
            if ws_bytes == 0:
                raise ValueError(f"dt_tsne_workspace_bytes rejects P={P}, n={n}, E={E4}")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            p_mat = torch.empty(P, n, n, **f64)
            status = torch.empty(P, dtype=torch.int32, device=dev)
            bs = (0, 0) if b is None else (b.stride(1), b.stride(0))
            check(lib.dt_tsne_affinities(ptr(a), n_a, a.stride(1), a.stride(0), ptr(b), n_b, bs[0], bs[1], P, E4,
                                         perplexity, ptr(p_mat), ptr(status), ptr(ws), ws_bytes, stream_ptr()),
                  "dt_tsne_affinities")
        else:
            p_mat = affinities.to(dev).contiguous()
            status = torch.isnan(p_mat[:, 0, 1]).to(torch.int32)
        if state is None:
            y0 = init.to(dev, torch.float64)
            y0 = y0.expand(P, n, 2) if y0.dim() == 2 else y0
            state = torch.zeros(P, tsne_state_doubles(n), **f64)
            views = tsne_state_views(state, n)
            views["y"].copy_(y0)
            views["gains"].fill_(1.0)
            views["ctl"][:, 0] = sys.float_info.max
        else:
            state = state.to(dev).clone()
        embedding = torch.empty(P, n, 2, dtype=torch.float32, device=dev)
        kl = torch.empty(P, **f64)
        check(lib.dt_tsne_descend(ptr(p_mat), P, n, ptr(state), it_begin, max_iter, ctypes.byref(prm), ptr(embedding),
                                  ptr(kl), stream_ptr()), "dt_tsne_descend")
        out = {"embedding": embedding, "kl_divergence": kl, "n_iter": state[:, 6 * n + 2].to(torch.int32),
               "status": status, "state": state}
    if return_affinities:
        out["affinities"] = p_mat
    return out


# ---------------------------------------------------------------------- trajectory alignment (include/dt_hip_align.h)
ALIGN_MAX_N = 1024
ALIGN_MAX_BAND = 1 << 20
ALIGN_DTW, ALIGN_FRECHET = 0, 1
ALIGN_OK, ALIGN_NONFINITE, ALIGN_NO_PATH = 0, 1, 2
_ALIGN_KINDS = {"dtw": ("dtw",), "frechet": ("frechet",), "both": ("dtw", "frechet")}


def _align_kinds(kind):
    if kind not in _ALIGN_KINDS:
        raise ValueError(f"kind={kind!r} must be one of {sorted(_ALIGN_KINDS)}")
    return _ALIGN_KINDS[kind]


def _align_band(band):
    band = _count(band, "band")
    if band > ALIGN_MAX_BAND:
        raise ValueError(f"band={band} must be at most {ALIGN_MAX_BAND}")
    return band


def _align_rows(t, name, layout):
    """[n, P, E] view of the rows of a trajectory tensor: step-major [n, S, ...] or, with layout "problem", [P, n, ...];
    a 2-D [n, E] tensor is one problem.  Unit stride along E, a copy only where the tensor has none."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if t.dim() < 2:
        raise ValueError(f"{name} must be [n, E], step-major [n, S, ...] or [P, n, ...], got shape {tuple(t.shape)}")
    if t.dim() == 2:
        t = t.unsqueeze(1)
    elif layout == "problem":
        t = t.transpose(0, 1)
    if t.dim() > 3:
        t = t.flatten(2)
    return t if t.stride(2) == 1 else t.contiguous()


def _align_shape(n_a, n_b, P):
    if not (2 <= n_a <= ALIGN_MAX_N and 2 <= n_b <= ALIGN_MAX_N):
        raise ValueError(f"an alignment needs 2 <= n <= {ALIGN_MAX_N} states on both sides, got {n_a} and {n_b}")
    if not 1 <= P <= 65535:
        raise ValueError(f"unsupported number of problems P={P}")


def _align_outputs(kinds, P, n_a, n_b, path, dev):
    out = {"status": torch.empty(P, dtype=torch.int32, device=dev)}
    for k in kinds:
        out[k] = torch.empty(P, dtype=torch.float64, device=dev)
        if path:
            out[f"{k}_path"] = torch.empty(P, n_a + n_b - 1, 2, dtype=torch.int32, device=dev)
            out[f"{k}_path_len"] = torch.empty(P, dtype=torch.int32, device=dev)
    return out


def device_align(X, Y, kind="both", band=0, path=True, cost=False, workspace_bytes=None, layout="step"):
    """DTW and / or the discrete Fréchet distance between the trajectories X [nX, S, ...] and Y [nY, S, ...] (step-major
    float32 device tensors, one problem per sample s, read in place; with ``layout="problem"`` [P, n, ...]): dt_align, the
    fp64 matrix of Euclidean distances between every state of X and every state of Y, then one dynamic programme per kind.
    ``kind``: "dtw", "frechet" or "both"; ``band``: 0, or a Sakoe-Chiba band in steps of the longer trajectory.
    Returns device tensors {dtw, frechet [S] fp64, status [S] int32 (0 ok, 1 non-finite input: the values are NaN, 2 no
    path)}, with ``path`` {dtw_path, frechet_path [S, nX+nY-1, 2] int32 (cells (i, j) from (0, 0), -1 past the length),
    dtw_path_len, frechet_path_len [S] int32}, and with ``cost`` the matrices cost [S, nX, nY] fp64.
    ``workspace_bytes``: a cap on the scratch; the problems then go through in chunks, with the same bits."""
    kinds = _align_kinds(kind)
    band = _align_band(band)
    if layout not in ("step", "problem"):
        raise ValueError(f"layout={layout!r} must be 'step' or 'problem'")
    a, b = _align_rows(X, "X", layout), _align_rows(Y, "Y", layout)
    (n_a, P, E), (n_b, Pb, Eb) = a.shape, b.shape
    if (P, E) != (Pb, Eb):
        raise ValueError(f"Y {tuple(Y.shape)} does not match X {tuple(X.shape)}: the same number of problems and the same "
                         "state size are needed")
    _align_shape(n_a, n_b, P)
    if not 1 <= E <= 1 << 28:
        raise ValueError(f"unsupported state size E={E}")
    path, cost = bool(path), bool(cost)
    lib = _hip.load()
    least = lib.dt_align_min_workspace_bytes(n_a, n_b, int(path), int(cost))
    ws_bytes = lib.dt_align_workspace_bytes(P, n_a, n_b, int(path), int(cost))
    if workspace_bytes is not None:
        if _count(workspace_bytes, "workspace_bytes") < least:
            raise ValueError(f"workspace_bytes={workspace_bytes} is below one problem's {least} bytes")
        ws_bytes = min(ws_bytes, int(workspace_bytes))
    _require_cuda(a, "X")
    _require_cuda(b, "Y")
    dev = a.device
    with torch.cuda.device(dev):
        out = _align_outputs(kinds, P, n_a, n_b, path, dev)
        if cost:
            out["cost"] = torch.empty(P, n_a, n_b, dtype=torch.float64, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        mask = sum(1 << (ALIGN_DTW if k == "dtw" else ALIGN_FRECHET) for k in kinds)
        check(lib.dt_align(ptr(a), n_a, a.stride(1), a.stride(0), ptr(b), n_b, b.stride(1), b.stride(0), P, E, mask, band,
                           ptr(out.get("cost")), ptr(out.get("dtw")), ptr(out.get("frechet")), ptr(out.get("dtw_path")),
                           ptr(out.get("dtw_path_len")), ptr(out.get("frechet_path")), ptr(out.get("frechet_path_len")),
                           ptr(out["status"]), ptr(ws), ws_bytes, stream_ptr()), "dt_align")
    return out


def device_align_cost_matrix(X, Y, layout="step"):
    """The cost matrices alone (dt_align_cost): {cost [S, nX, nY] fp64, status [S] int32} for X and Y as in ``device_align``."""
    if layout not in ("step", "problem"):
        raise ValueError(f"layout={layout!r} must be 'step' or 'problem'")
    a, b = _align_rows(X, "X", layout), _align_rows(Y, "Y", layout)
    (n_a, P, E), (n_b, Pb, Eb) = a.shape, b.shape
    if (P, E) != (Pb, Eb):
        raise ValueError(f"Y {tuple(Y.shape)} does not match X {tuple(X.shape)}")
    _align_shape(n_a, n_b, P)
    if not 1 <= E <= 1 << 28:
        raise ValueError(f"unsupported state size E={E}")
    _require_cuda(a, "X")
    _require_cuda(b, "Y")
    lib = _hip.load()
    with torch.cuda.device(a.device):
        out = {"cost": torch.empty(P, n_a, n_b, dtype=torch.float64, device=a.device),
               "status": torch.empty(P, dtype=torch.int32, device=a.device)}
        check(lib.dt_align_cost(ptr(a), n_a, a.stride(1), a.stride(0), ptr(b), n_b, b.stride(1), b.stride(0), P, E,
                                ptr(out["cost"]), ptr(out["status"]), stream_ptr()), "dt_align_cost")
    return out


def device_align_cost(cost, kind="both", band=0, path=True):
    """The dynamic programmes of ``device_align`` on caller-made cost matrices [P, n_a, n_b] (or [n_a, n_b]) fp64 on the
    device, for instance LPIPS between steps: dt_align_dp per kind.  The same outputs, without ``cost``; a NaN or Inf
    entry gives status 1."""
    kinds = _align_kinds(kind)
    band = _align_band(band)
    if not isinstance(cost, torch.Tensor) or cost.dtype != torch.float64 or cost.dim() not in (2, 3):
        raise ValueError("cost must be a float64 tensor [P, n_a, n_b] or [n_a, n_b]")
    if cost.dim() == 2:
        cost = cost.unsqueeze(0)
    P, n_a, n_b = cost.shape
    _align_shape(n_a, n_b, P)
    path = bool(path)
    _require_cuda(cost, "cost")
    lib = _hip.load()
    cost = cost.contiguous()
    dev = cost.device
    with torch.cuda.device(dev):
        out = _align_outputs(kinds, P, n_a, n_b, path, dev)
        ws_bytes = lib.dt_align_workspace_bytes(P, n_a, n_b, int(path), 1)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        for k in kinds:
            check(lib.dt_align_dp(ptr(cost), P, n_a, n_b, ALIGN_DTW if k == "dtw" else ALIGN_FRECHET, band, ptr(out[k]),
                                  ptr(out.get(f"{k}_path")), ptr(out.get(f"{k}_path_len")), ptr(out["status"]), ptr(ws),
                                  ws_bytes, stream_ptr()), "dt_align_dp")
    return out


# ---------------------------------------------------------------------- layer-wise CKA (include/dt_hip_cka.h)
CKA_MIN_N, CKA_MAX_N, CKA_MAX_LAYERS, CKA_MAX_P, CKA_SLAB = 4, 2048, 64, 1 << 24, 1024
CKA_SUM_ROWS = 8
CKA_SUMS = CKA_SUM_ROWS + CKA_MAX_N
CKA_NONFINITE, CKA_ZERO_VARIANCE, CKA_SELF_NOT_POSITIVE = 1, 2, 4


class PitchedFeatures:
    """A layer of n feature rows inside a wider buffer: ``view`` [n, h, w, cp] float32 (NHWC, channels padded to cp, the
    three inner axes dense, any row stride) of which the first ``c`` channels of every pixel are the features.  The pad
    channels are never read.  ``UNetHandle.block_features`` returns these over the forward's workspace."""

    def __init__(self, view, c):
        if not isinstance(view, torch.Tensor) or view.dtype != torch.float32 or view.dim() != 4:
            raise ValueError("PitchedFeatures: view must be a float32 tensor [n, h, w, cp]")
        n, h, w, cp = view.shape
        if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 1 <= c <= cp:
            raise ValueError(f"PitchedFeatures: c={c!r} must be an int in [1, {cp}]")
        if view.stride()[1:] != (w * cp, cp, 1):
            raise ValueError(f"PitchedFeatures: the inner axes of view must be dense, got strides {view.stride()}")
        self.view, self.c = view, int(c)

    @property
    def n(self):
        return self.view.shape[0]

    def dense(self):
        """[n, h*w*c] copy without the pad channels (feature k = pixel * c + channel, the order the Gram walks)."""
        return self.view[..., :self.c].reshape(self.n, -1)


class CkaGrams(collections.namedtuple("CkaGrams", "gram sums status n")):
    """``device_cka_gram``'s result, all on the device: gram [L, n, n] and sums [L, CKA_SUMS] float64, status [L] int32."""
    __slots__ = ()


def _cka_layers(layers, name):
    """[(tensor kept alive, row stride, groups, c, pitch)] and n of a list of layers, each checked"""
    if isinstance(layers, (torch.Tensor, PitchedFeatures)):
        layers = [layers]
    try:
        layers = list(layers)
    except TypeError:
        raise ValueError(f"{name} must be a list of layers") from None
    if not 1 <= len(layers) <= CKA_MAX_LAYERS:
        raise ValueError(f"{name} must hold 1 .. {CKA_MAX_LAYERS} layers, got {len(layers)}")
    out, n = [], None
    for i, layer in enumerate(layers):
        if isinstance(layer, PitchedFeatures):
            v = layer.view
            desc = (v, v.stride(0), v.shape[1] * v.shape[2], layer.c, v.shape[3])
        elif isinstance(layer, torch.Tensor):
            if layer.dtype != torch.float32 or layer.dim() < 2:
                raise ValueError(f"{name}[{i}] must be a float32 tensor [n, ...], got {tuple(layer.shape)} {layer.dtype}")
            v = layer.flatten(1)
            if v.shape[1] > 1 and v.stride(1) != 1:
                v = v.contiguous()
            desc = (v, v.stride(0), 1, v.shape[1], v.shape[1])
        else:
            raise ValueError(f"{name}[{i}] must be a torch tensor or PitchedFeatures, got {type(layer).__name__}")
        if not 1 <= desc[2] * desc[3] <= CKA_MAX_P:
            raise ValueError(f"{name}[{i}] has {desc[2] * desc[3]} features, 1 .. {CKA_MAX_P} are supported")
        if desc[1] < 0:
            raise ValueError(f"{name}[{i}] has a negative row stride")
        if n is None:
            n = v.shape[0]
        elif v.shape[0] != n:
            raise ValueError(f"{name}[{i}] has {v.shape[0]} rows, the layers before it {n}: CKA compares the same inputs")
        out.append(desc)
    if not CKA_MIN_N <= n <= CKA_MAX_N:
        raise ValueError(f"CKA needs {CKA_MIN_N} <= n <= {CKA_MAX_N} rows, got {n}")
    return out, n


def _cka_workspace_bytes(workspace_bytes):
    return None if workspace_bytes is None else _count(workspace_bytes, "workspace_bytes")


def device_cka_gram(layers, workspace_bytes=None):
    """Feature-centred fp64 Grams of a list of layers over the same n inputs (dt_cka_gram).  A layer is a float32 device
    tensor [n, ...] (trailing axes flattened, row stride honoured, no copy where the trailing axes are dense) or a
    ``PitchedFeatures``.  Returns ``CkaGrams`` (gram, sums, status, n), all on the device.  ``workspace_bytes``: a cap on
    the scratch; a layer's slabs then take turns, with the same bits."""
    descs, n = _cka_layers(layers, "layers")
    cap = _cka_workspace_bytes(workspace_bytes)
    L, p_max = len(descs), max(d[2] * d[3] for d in descs)
    lib = _hip.load()
    ws_bytes = lib.dt_cka_workspace_bytes(L, n, p_max)
    if cap is not None:
        least = lib.dt_cka_min_workspace_bytes(n, p_max)
        if cap < least:
            raise ValueError(f"workspace_bytes={cap} is below the {least} bytes that the means and one slab take")
        ws_bytes = min(ws_bytes, cap)
    for d in descs:
        _require_cuda(d[0], "a CKA layer")
    dev = descs[0][0].device
    if any(d[0].device != dev for d in descs):
        raise ValueError("the layers must live on one device")
    base = (c_void_p * L)(*[d[0].data_ptr() for d in descs])
    rs = (ctypes.c_longlong * L)(*[d[1] for d in descs])
    groups, c, pitch = ((c_int * L)(*[d[k] for d in descs]) for k in (2, 3, 4))
    with torch.cuda.device(dev):
        out = CkaGrams(torch.empty(L, n, n, dtype=torch.float64, device=dev),
                       torch.empty(L, CKA_SUMS, dtype=torch.float64, device=dev),
                       torch.empty(L, dtype=torch.int32, device=dev), n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        check(lib.dt_cka_gram(base, rs, groups, c, pitch, L, n, ptr(out.gram), ptr(out.sums), ptr(out.status), ptr(ws),
                              ws_bytes, stream_ptr()), "dt_cka_gram")
    return out


def _cka_grams_check(g, name):
    L = g.gram.shape[0] if isinstance(g.gram, torch.Tensor) and g.gram.dim() == 3 else -1
    ok = (L >= 1 and g.gram.dtype == torch.float64 and tuple(g.gram.shape) == (L, g.n, g.n) and g.gram.is_contiguous()
          and isinstance(g.sums, torch.Tensor) and g.sums.dtype == torch.float64 and tuple(g.sums.shape) == (L, CKA_SUMS)
          and g.sums.is_contiguous() and isinstance(g.status, torch.Tensor) and g.status.dtype == torch.int32
          and tuple(g.status.shape) == (L,))
    if not ok or not 1 <= L <= CKA_MAX_LAYERS or not CKA_MIN_N <= g.n <= CKA_MAX_N:
        raise ValueError(f"{name} is not a CkaGrams of device_cka_gram")


def device_cka(a, b=None, workspace_bytes=None):
    """Linear CKA, biased and debiased, between every layer of ``a`` and every layer of ``b`` (``b=None``: of ``a``
    itself).  ``a`` and ``b`` are lists of layers as ``device_cka_gram`` takes them, or its ``CkaGrams`` results, so that
    one side's Grams are made once and scored many times.  Returns device tensors {cka, cka_unbiased [La, Lb] float64,
    hsic [La, Lb, 2] float64 (the two numerators), status_a [La], status_b [Lb] int32 (bits CKA_NONFINITE,
    CKA_ZERO_VARIANCE, CKA_SELF_NOT_POSITIVE; a score that involves a flagged layer is NaN for the estimator concerned)}.
    The contract is in include/dt_hip_cka.h."""
    sides = []
    for side, name in ((a, "a"), (b, "b")):
        if side is None and name == "b":
            sides.append(None)
        elif isinstance(side, CkaGrams):
            _cka_grams_check(side, name)
            sides.append(side)
        else:
            sides.append(_cka_layers(side, name))
    n = [s.n if isinstance(s, CkaGrams) else s[1] for s in sides if s is not None]
    if len(set(n)) != 1:
        raise ValueError(f"a has {n[0]} rows and b {n[1]}: CKA compares features of the same inputs")
    _cka_workspace_bytes(workspace_bytes)
    ga = a if isinstance(a, CkaGrams) else device_cka_gram(a, workspace_bytes)
    gb = ga if b is None else (b if isinstance(b, CkaGrams) else device_cka_gram(b, workspace_bytes))
    for g in (ga, gb):
        _require_cuda(g.gram, "a CKA Gram")
    if gb.gram.device != ga.gram.device:
        raise ValueError("a and b must live on one device")
    La, Lb, dev = ga.gram.shape[0], gb.gram.shape[0], ga.gram.device
    with torch.cuda.device(dev):
        out = {"cka": torch.empty(La, Lb, dtype=torch.float64, device=dev),
               "cka_unbiased": torch.empty(La, Lb, dtype=torch.float64, device=dev),
               "hsic": torch.empty(La, Lb, 2, dtype=torch.float64, device=dev), "status_a": ga.status, "status_b": gb.status}
        check(_hip.load().dt_cka_scores(ptr(ga.gram), ptr(ga.sums), ptr(ga.status), La, ptr(gb.gram), ptr(gb.sums),
                                        ptr(gb.status), Lb, n[0], ptr(out["cka"]), ptr(out["cka_unbiased"]), ptr(out["hsic"]),
                                        stream_ptr()), "dt_cka_scores")
    return out


# ---------------------------------------------------------------------- spatial-frequency spectra (include/dt_hip_spectral.h)
SPECTRAL_MAX_HW, SPECTRAL_MAX_C, SPECTRAL_MAX_BINS, SPECTRAL_MAX_ROWS = 64, 64, 256, 1 << 24
SPECTRAL_PAIR_K = 5
SPECTRAL_PA, SPECTRAL_PB, SPECTRAL_CRE, SPECTRAL_CIM, SPECTRAL_D = range(5)
SPECTRAL_OK, SPECTRAL_NONFINITE = 0, 1
_RADIAL_TABLES = {}


def _spectral_picture(C, H, W):
    C, H, W = _count(C, "C", 1), _count(H, "H", 1), _count(W, "W", 1)
    if C > SPECTRAL_MAX_C or H > SPECTRAL_MAX_HW or W > SPECTRAL_MAX_HW:
        raise ValueError(f"a spectrum takes C <= {SPECTRAL_MAX_C} and H, W <= {SPECTRAL_MAX_HW}, got C={C}, H={H}, W={W}")
    return C, H, W


def radial_bins(H, W):
    """(table int32 [H, W], cells_per_bin int64 [n_bins]) of the radial binning of an H x W spectrum.  Coefficient (u, v)
    has the signed frequencies fu = min(u, H - u), fv = min(v, W - v) and the radius r, in cycles per max(H, W) pixels,
    r^2 = (fu M / H)^2 + (fv M / W)^2 with M = max(H, W); its bin is round(r) (halves up), decided in integers:
    bin = #{b >= 0 : (2b + 1)^2 (HW)^2 <= 4 r^2 (HW)^2}, so that no table depends on libm.  DC is alone in bin 0, the table
    is symmetric under (u, v) -> (-u, -v), and n_bins = max bin + 1."""
    _, H, W = _spectral_picture(1, H, W)
    M = max(H, W)
    fu = np.minimum(np.arange(H), H - np.arange(H)).astype(np.int64)
    fv = np.minimum(np.arange(W), W - np.arange(W)).astype(np.int64)
    q = 4 * ((fu[:, None] * M * W) ** 2 + (fv[None, :] * M * H) ** 2)       # 4 r^2 (HW)^2 < 2^40
    table = np.zeros((H, W), dtype=np.int64)
    b = 0
    while True:
        above = q >= (2 * b + 1) ** 2 * (H * W) ** 2
        if not above.any():
            break
        table += above
        b += 1
    return table.astype(np.int32), np.bincount(table.ravel())


def _spectral_bins(bins, H, W):
    """``bins`` as a host table int32 [H, W] and its n_bins, checked (None: None, the radial table)"""
    if bins is None:
        return None
    host = bins.detach().cpu().numpy() if isinstance(bins, torch.Tensor) else np.asarray(bins)
    if host.shape != (H, W):
        raise ValueError(f"bins must be a table [H, W] = [{H}, {W}], got shape {tuple(host.shape)}")
    if host.dtype.kind not in "iu":
        raise ValueError(f"bins must hold integers, got {host.dtype}")
    low, high = int(host.min()), int(host.max())
    if low < -1 or high < 0 or high >= SPECTRAL_MAX_BINS:
        raise ValueError(f"bins must hold -1 (left out) or a bin in [0, {SPECTRAL_MAX_BINS}) and name at least one bin, "
                         f"got values in [{low}, {high}]")
    return np.ascontiguousarray(host.astype(np.int32)), high + 1


def _spectral_table(bins, H, W, device):
    """(device table int32 [H, W], n_bins) of what ``_spectral_bins`` returned (the radial table is kept per shape and device)"""
    if bins is not None:
        return torch.from_numpy(bins[0]).to(device), bins[1]
    key = (H, W, str(device))
    if key not in _RADIAL_TABLES:
        table, cells = radial_bins(H, W)
        _RADIAL_TABLES[key] = (torch.from_numpy(table).to(device), len(cells))
    return _RADIAL_TABLES[key]


def _spectral_rows(t, name, E):
    """(tensor, leading shape, n_outer, n_inner, outer stride, inner stride) of a set of rows of E floats: [n, S, E]
    (contiguous or a view: a slice of the sample axis, every k-th state) or flat [Q, E]; read in place when the rows
    themselves are contiguous, copied otherwise"""
    t = _f32_rows(t, name, "[n, S, E] or [Q, E]")
    if t.shape[-1] != E:
        raise ValueError(f"{name} has rows of {t.shape[-1]} floats, C*H*W = {E} are needed")
    if t.numel() == 0 or t.numel() // E > SPECTRAL_MAX_ROWS:
        raise ValueError(f"{name} must hold between 1 and {SPECTRAL_MAX_ROWS} rows, got shape {tuple(t.shape)}")
    if E > 1 and t.stride(-1) != 1:
        t = t.contiguous()
    if t.dim() == 2:
        return t, (t.shape[0],), 1, t.shape[0], 0, t.stride(0)
    return t, tuple(t.shape[:2]), t.shape[0], t.shape[1], t.stride(0), t.stride(1)


def _spectral_sum(lib, out, status, n_outer, n_inner, C, n_bins, K):
    sums = torch.empty(n_outer, C, n_bins, K, dtype=torch.float64, device=out.device)
    count = torch.empty(n_outer, dtype=torch.int32, device=out.device)
    check(lib.dt_spectral_sum(ptr(out), ptr(status), n_outer, n_inner, C, n_bins, K, ptr(sums), ptr(count), stream_ptr()),
          "dt_spectral_sum")
    return sums, count


def device_spectrum(X, C, H, W, bins=None, sum_samples=False, workspace_bytes=None):
    """Per-band power spectrum of the pictures of X: [n, S, E] (a trajectory or a view of one) or [Q, E], float32 on the
    device, E = C*H*W in NCHW order, read in place (dt_spectral_power: the unnormalised fp64 DFT of every channel, |F|^2
    summed over the cells of each bin).  ``bins``: an integer table [H, W] of bin numbers, -1 for a coefficient that is
    left out; None: ``radial_bins(H, W)``.  Returns device tensors {power [.., C, n_bins] fp64, status [..] int32 (0 ok,
    1 a NaN or Inf in the row: its outputs are NaN)}, [..] being [n, S] or [Q]; with ``sum_samples`` power is
    [n, C, n_bins] (or [C, n_bins]), summed over the samples in index order without the flagged rows, and count [n] (or
    a scalar) says how many were added.  ``workspace_bytes``: a larger scratch than needed; it changes nothing."""
    return _spectral_call(X, None, C, H, W, bins, sum_samples, workspace_bytes)


def device_spectral_pair(X, Y, C, H, W, bins=None, sum_samples=False, workspace_bytes=None):
    """Per-band spectra of a teacher set X against a student set Y of the same shape (each as in ``device_spectrum``, with
    strides of its own): dt_spectral_pair.  With A = DFT(x), B = DFT(y) and Delta = DFT(double(x) - double(y)) per
    channel, returns device tensors {power_a = sum |A|^2, power_b = sum |B|^2, error = sum |Delta|^2 [.., C, n_bins],
    cross [.., C, n_bins, 2] = sum A conj(B) (real, imaginary), status [..]}, all fp64 sums over the cells of a bin;
    ``sum_samples`` as in ``device_spectrum``, with count."""
    if Y is None:
        raise ValueError("Y must be a torch tensor, got None")
    return _spectral_call(X, Y, C, H, W, bins, sum_samples, workspace_bytes)


def _spectral_call(X, Y, C, H, W, bins, sum_samples, workspace_bytes):
    C, H, W = _spectral_picture(C, H, W)
    E = C * H * W
    bins = _spectral_bins(bins, H, W)
    if workspace_bytes is not None:
        _count(workspace_bytes, "workspace_bytes")
    a, lead, n_outer, n_inner, a_os, a_is = _spectral_rows(X, "X", E)
    pair = Y is not None
    if pair:
        b, lead_b, _, _, b_os, b_is = _spectral_rows(Y, "Y", E)
        if lead_b != lead:
            raise ValueError(f"Y {tuple(Y.shape)} does not match X {tuple(X.shape)}")
    for t, name in ((a, "X"), (b, "Y")) if pair else ((a, "X"),):
        if not t.is_cuda:
            raise ValueError(f"{name} must be on the device, got {t.device}: the MI355X path has no CPU fallback")
    if pair and b.device != a.device:
        raise ValueError(f"X is on {a.device}, Y on {b.device}")
    dev = a.device
    with torch.cuda.device(dev):
        table, n_bins = _spectral_table(bins, H, W, dev)
        lib = _hip.load()
        need = lib.dt_spectral_workspace_bytes(H, W, n_bins)
        if workspace_bytes is not None and workspace_bytes < need:
            raise ValueError(f"workspace_bytes={workspace_bytes} is below the {need} bytes a {H} x {W} table needs")
        ws_bytes = need if workspace_bytes is None else int(workspace_bytes)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        rows, K = n_outer * n_inner, SPECTRAL_PAIR_K if pair else 1
        out = torch.empty(rows, C, n_bins, K, dtype=torch.float64, device=dev)
        status = torch.empty(rows, dtype=torch.int32, device=dev)
        tail = (n_outer, n_inner, C, H, W, ptr(table), n_bins, ptr(out), ptr(status), ptr(ws), ws_bytes, stream_ptr())
        if pair:
            check(lib.dt_spectral_pair(ptr(a), a_os, a_is, ptr(b), b_os, b_is, *tail), "dt_spectral_pair")
        else:
            check(lib.dt_spectral_power(ptr(a), a_os, a_is, *tail), "dt_spectral_power")
        res = {"status": status.view(lead)}
        if sum_samples:
            out, count = _spectral_sum(lib, out, status, n_outer, n_inner, C, n_bins, K)
            lead = lead[:-1]
            res["count"] = count.view(lead)
        v = out.view(lead + (C, n_bins, K))
        if pair:
            res.update(power_a=v[..., SPECTRAL_PA], power_b=v[..., SPECTRAL_PB], cross=v[..., SPECTRAL_CRE:SPECTRAL_CIM + 1],
                       error=v[..., SPECTRAL_D])
        else:
            res["power"] = v[..., 0]
    return res


# ---------------------------------------------------------------------- sliced Wasserstein distance (include/dt_hip_swd.h)
SWD_MAX_N, SWD_MAX_E, SWD_MAX_L, SWD_MAX_P = 2048, 1 << 20, 4096, 1 << 16
SWD_OK, SWD_NONFINITE = 0, 1
SWD_SORTED_WORKSPACE_BYTES = 256
_SWD_DIRECTIONS = {}            # (E, L, seed) -> float32 [L, E] on the host
_SWD_DEVICE_DIRECTIONS = {}     # (E, L, seed, device) -> the same on a device


class SwdSorted(collections.namedtuple("SwdSorted", "sorted status n directions")):
    """``device_swd_sorted``'s result: sorted [P, L, n] float64 and status [P] int32 on the device, the rows per set ``n``
    and the device tensor of directions [L, E] the projections were made with."""
    __slots__ = ()


def swd_directions(E, L, seed=0):
    """L directions in R^E for ``device_swd``: float32 [L, E] on the host.  Drawn as float64 normals from a torch CPU
    generator of their own seeded with ``seed`` (the global generator is neither read nor advanced), every row divided by
    its float64 norm and then rounded to float32, so a row's norm is 1 to float32 rounding.  Kept per (E, L, seed): the
    same tensor comes back, and must not be written to."""
    E, L, seed = _count(E, "E", 1), _count(L, "L", 1), _count(seed, "seed")
    if E > SWD_MAX_E or L > SWD_MAX_L:
        raise ValueError(f"directions take E <= {SWD_MAX_E} and L <= {SWD_MAX_L}, got E={E}, L={L}")
    key = (E, L, seed)
    if key not in _SWD_DIRECTIONS:
        gen = torch.Generator(device="cpu")
        gen.manual_seed(seed)
        d = torch.randn(L, E, dtype=torch.float64, generator=gen)
        _SWD_DIRECTIONS[key] = (d / d.norm(dim=1, keepdim=True)).to(torch.float32)
    return _SWD_DIRECTIONS[key]


def _swd_rows(t, name):
    """(tensor, P, n, E, problem stride, row stride) of a set of rows per state: [P, n, E] (contiguous or a view) or one
    set [n, E] (P = 1); read in place when the rows themselves are contiguous, copied otherwise"""
    t = _f32_rows(t, name, "[states, n, E] or [n, E]")
    E, n = t.shape[-1], t.shape[-2]
    P = t.shape[0] if t.dim() == 3 else 1
    if not (1 <= n <= SWD_MAX_N and 1 <= E <= SWD_MAX_E and 1 <= P <= SWD_MAX_P):
        raise ValueError(f"{name} must hold 1 .. {SWD_MAX_P} states of 1 .. {SWD_MAX_N} rows of 1 .. {SWD_MAX_E} floats, "
                         f"got shape {tuple(t.shape)}")
    if (E > 1 and t.stride(-1) != 1) or any(s < 0 for s in t.stride()):
        t = t.contiguous()
    return (t, P, n, E, t.stride(0), t.stride(1)) if t.dim() == 3 else (t, 1, n, E, 0, t.stride(0))


def _swd_theta(directions, E=None):
    """directions as given: a float32 tensor [L, E] with unit column stride, on any device"""
    if not isinstance(directions, torch.Tensor) or directions.dtype != torch.float32 or directions.dim() != 2:
        raise ValueError("directions must be a float32 torch tensor [L, E]")
    L, Ed = directions.shape
    if not 1 <= L <= SWD_MAX_L or not 1 <= Ed <= SWD_MAX_E:
        raise ValueError(f"directions must be [L, E] with L <= {SWD_MAX_L} and E <= {SWD_MAX_E}, got {tuple(directions.shape)}")
    if E is not None and Ed != E:
        raise ValueError(f"the directions live in R^{Ed}, the rows in R^{E}")
    if (Ed > 1 and directions.stride(1) != 1) or directions.stride(0) < 0:
        directions = directions.contiguous()
    return directions


def _swd_sorted_check(s, name):
    ok = (isinstance(s.sorted, torch.Tensor) and s.sorted.dtype == torch.float64 and s.sorted.dim() == 3 and s.sorted.is_contiguous()
          and isinstance(s.status, torch.Tensor) and s.status.dtype == torch.int32 and s.status.is_contiguous()
          and isinstance(s.directions, torch.Tensor) and s.directions.dtype == torch.float32 and s.directions.dim() == 2
          and not isinstance(s.n, bool) and isinstance(s.n, (int, np.integer)))
    if ok:
        P, L, n = s.sorted.shape
        ok = (n == s.n and 1 <= n <= SWD_MAX_N and 1 <= L <= SWD_MAX_L and 1 <= P <= SWD_MAX_P and tuple(s.status.shape) == (P,)
              and s.directions.shape[0] == L and s.status.device == s.sorted.device == s.directions.device)
    if not ok:
        raise ValueError(f"{name} is not a SwdSorted of device_swd_sorted")


def _same_directions(x, y):
    return x is y or (x.data_ptr() == y.data_ptr() and x.shape == y.shape and x.stride() == y.stride() and x.device == y.device)


def _on_device(t, name):
    if not t.is_cuda:
        raise ValueError(f"{name} must be on the device, got {t.device}: the MI355X path has no CPU fallback")


def device_swd_sorted(X, directions):
    """Sorted projections of the sets of X onto ``directions`` (dt_swd_sorted): X is float32 on the device, [P, n, E] (one
    set of n rows per state; views are read in place) or [n, E]; ``directions`` float32 [L, E] (``swd_directions``, or the
    caller's own; a host tensor is copied to X's device).  Returns ``SwdSorted`` (sorted [P, L, n] float64 ascending along
    n, status [P] int32: 1 for a NaN or Inf in the state's rows or in the directions, its columns are then NaN).  Hand the
    result to ``device_swd`` in place of the tensor to compare one set with many others."""
    x, P, n, E, ps, rs = _swd_rows(X, "X")
    theta = _swd_theta(directions, E)
    _on_device(x, "X")
    dev = x.device
    if theta.device != dev:
        theta = theta.to(dev)
    L = theta.shape[0]
    with torch.cuda.device(dev):
        out = SwdSorted(torch.empty(P, L, n, dtype=torch.float64, device=dev), torch.empty(P, dtype=torch.int32, device=dev),
                        n, theta)
        ws = torch.empty(SWD_SORTED_WORKSPACE_BYTES, dtype=torch.uint8, device=dev)
        check(_hip.load().dt_swd_sorted(ptr(x), ps, rs, n, E, ptr(theta), theta.stride(0), L, P, ptr(out.sorted),
                                        ptr(out.status), ptr(ws), SWD_SORTED_WORKSPACE_BYTES, stream_ptr()), "dt_swd_sorted")
    return out


def device_swd(a, b, directions=None, n_directions=512, p=2, seed=0, per_direction=False, workspace_bytes=None):
    """Sliced Wasserstein distance between the sets of ``a`` and of ``b``, state by state (dt_swd, or dt_swd_distance when
    a side comes sorted).  A side is a float32 device tensor [P, n, E] (one set of n rows per state; n may differ between
    the sides; views are read in place) or [n, E], or the ``SwdSorted`` of ``device_swd_sorted``; a side with one state is
    shared by all states of the other.  ``directions``: float32 [L, E]; None: those a sorted side was made with, else
    ``swd_directions(E, n_directions, seed)``.  A sorted side made with other directions is refused.
    Returns device tensors {mean_w [P] float64 (the mean over the directions of W_p^p), max_w [P] (the largest), argmax [P]
    int32 (the first direction that reaches it), status [P] int32 (1: a NaN or Inf in the state's rows or the directions;
    its outputs are NaN, argmax -1)} and, with ``per_direction``, w [P, L].  The p-th root is the caller's (float64).
    ``workspace_bytes``: a cap on the scratch of dt_swd; the states then take turns, with the same bits.  The contract is
    in include/dt_hip_swd.h."""
    if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or p not in (1, 2):
        raise ValueError(f"p={p!r} must be 1 or 2")
    cap = None if workspace_bytes is None else _count(workspace_bytes, "workspace_bytes")
    sides = []
    for side, name in ((a, "a"), (b, "b")):
        if isinstance(side, SwdSorted):
            _swd_sorted_check(side, name)
            sides.append(None)
        else:
            sides.append(_swd_rows(side, name))
    widths = {s[3] for s in sides if s is not None} | {s.directions.shape[1] for s in (a, b) if isinstance(s, SwdSorted)}
    if len(widths) != 1:
        raise ValueError(f"a and b must have rows of one width, got {sorted(widths)}")
    E = widths.pop()
    made = [s.directions for s in (a, b) if isinstance(s, SwdSorted)]
    if directions is not None:
        theta = _swd_theta(directions, E)
    elif made:
        theta = made[0]
    else:
        theta = swd_directions(E, _count(n_directions, "n_directions", 1), seed)
    if any(not _same_directions(m, theta) for m in made):
        raise ValueError("a sorted side was made with other directions than the ones given")
    counts = [s.sorted.shape[0] if isinstance(s, SwdSorted) else r[1] for s, r in zip((a, b), sides)]
    P = max(counts)
    if any(c not in (1, P) for c in counts):
        raise ValueError(f"a has {counts[0]} states and b {counts[1]}: equal numbers, or one state on a side")
    tensors = [s.sorted if isinstance(s, SwdSorted) else r[0] for s, r in zip((a, b), sides)]
    for t, name in zip(tensors, ("a", "b")):
        _on_device(t, name)
    dev = tensors[0].device
    if tensors[1].device != dev:
        raise ValueError(f"a is on {dev}, b on {tensors[1].device}")
    if theta.device != dev:      # (not with a sorted side: its directions are where it is)
        key = (E, theta.shape[0], seed, str(dev))
        if directions is None:
            if key not in _SWD_DEVICE_DIRECTIONS:
                _SWD_DEVICE_DIRECTIONS[key] = theta.to(dev)
            theta = _SWD_DEVICE_DIRECTIONS[key]
        else:
            theta = theta.to(dev)
    L = theta.shape[0]
    lib = _hip.load()
    n_a, n_b = (s.n if isinstance(s, SwdSorted) else r[2] for s, r in zip((a, b), sides))
    if not made:
        least, ws_bytes = lib.dt_swd_workspace_bytes(1, n_a, n_b, L), lib.dt_swd_workspace_bytes(P, n_a, n_b, L)
        if cap is not None:
            if cap < least:
                raise ValueError(f"workspace_bytes={cap} is below the {least} bytes that one state takes")
            ws_bytes = min(ws_bytes, cap)
    else:
        ws_bytes = lib.dt_swd_distance_workspace_bytes(P, L)
    with torch.cuda.device(dev):
        res = {"mean_w": torch.empty(P, dtype=torch.float64, device=dev), "max_w": torch.empty(P, dtype=torch.float64, device=dev),
               "argmax": torch.empty(P, dtype=torch.int32, device=dev), "status": torch.empty(P, dtype=torch.int32, device=dev)}
        w = torch.empty(P, L, dtype=torch.float64, device=dev) if per_direction else None
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        outs = (ptr(w) if per_direction else None, ptr(res["mean_w"]), ptr(res["max_w"]), ptr(res["argmax"]), ptr(res["status"]),
                ptr(ws), ws_bytes, stream_ptr())
        if not made:
            (xa, Pa, _, _, a_ps, a_rs), (xb, Pb, _, _, b_ps, b_rs) = sides
            check(lib.dt_swd(ptr(xa), a_ps if Pa == P else 0, a_rs, n_a, ptr(xb), b_ps if Pb == P else 0, b_rs, n_b, E,
                             ptr(theta), theta.stride(0), L, P, p, *outs), "dt_swd")
        else:
            sa, sb = (s if isinstance(s, SwdSorted) else device_swd_sorted(s, theta) for s in (a, b))
            stride = lambda s: s.sorted.stride(0) if s.sorted.shape[0] == P and P > 1 else 0
            check(lib.dt_swd_distance(ptr(sa.sorted), stride(sa), ptr(sa.status), n_a, ptr(sb.sorted), stride(sb), ptr(sb.status),
                                      n_b, L, P, p, *outs), "dt_swd_distance")
        if per_direction:
            res["w"] = w
    return res


# ---------------------------------------------------------------------- entropic transport cost (include/dt_hip_sinkhorn.h)
SINKHORN_MAX_N, SINKHORN_MAX_E, SINKHORN_MAX_P, SINKHORN_MAX_ITER = 2048, 1 << 20, 1 << 16, 10000
SINKHORN_OK, SINKHORN_NONFINITE, SINKHORN_BAD_EPS, SINKHORN_NOT_CONVERGED = 0, 1, 2, 4
SINKHORN_DEFAULT_MAX_ITER, SINKHORN_DEFAULT_TOL = 300, 1e-6


def _sinkhorn_p(p):
    if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or p not in (1, 2):
        raise ValueError(f"p={p!r} must be 1 or 2")
    return int(p)


def _sinkhorn_sides(a, b):
    """the two row sets of a Sinkhorn call ((tensor, P, n, E, problem stride, row stride) each, as ``_swd_rows`` gives them;
    a side with one state has problem stride 0) and the number of problems; every error a ValueError, the device last"""
    sides = [_swd_rows(a, "a"), _swd_rows(b, "b")]
    if sides[0][3] != sides[1][3]:
        raise ValueError(f"a and b must have rows of one width, got {sides[0][3]} and {sides[1][3]}")
    P = max(sides[0][1], sides[1][1])
    if any(s[1] not in (1, P) for s in sides):
        raise ValueError(f"a has {sides[0][1]} states and b {sides[1][1]}: equal numbers, or one state on a side")
    return [(t, Ps, n, E, ps if Ps == P and P > 1 else 0, rs) for t, Ps, n, E, ps, rs in sides], P


def _sinkhorn_devices(sides):
    for (t, *_), name in zip(sides, ("a", "b")):
        _on_device(t, name)
    if sides[0][0].device != sides[1][0].device:
        raise ValueError(f"a is on {sides[0][0].device}, b on {sides[1][0].device}")
    return sides[0][0].device


def _sinkhorn_workspace(lib, P, n_a, n_b, cap):
    least, ws_bytes = lib.dt_sinkhorn_workspace_bytes(1, n_a, n_b), lib.dt_sinkhorn_workspace_bytes(P, n_a, n_b)
    if cap is not None:
        if cap < least:
            raise ValueError(f"workspace_bytes={cap} is below the {least} bytes that one state takes")
        ws_bytes = min(ws_bytes, cap)
    return ws_bytes


def device_sinkhorn_mean_cost(a, b, p=2, workspace_bytes=None):
    """Mean over all pairs (i, j) of the cost C_ij = |a_i - b_j|^p between the sets of ``a`` and of ``b``, state by state
    (dt_sinkhorn_mean_cost): float32 device tensors [P, n, E] or [n, E] as ``device_swd`` takes them (views are read in
    place; a side with one state is shared by all states of the other).  Returns {mean_cost [P] float64, status [P] int32
    (1: a NaN or Inf in the state's rows, its mean is NaN)} on the device: what an epsilon is made from without a host
    round trip."""
    p = _sinkhorn_p(p)
    cap = None if workspace_bytes is None else _count(workspace_bytes, "workspace_bytes")
    sides, P = _sinkhorn_sides(a, b)
    dev = _sinkhorn_devices(sides)
    (xa, _, n_a, E, a_ps, a_rs), (xb, _, n_b, _, b_ps, b_rs) = sides
    lib = _hip.load()
    ws_bytes = _sinkhorn_workspace(lib, P, n_a, n_b, cap)
    with torch.cuda.device(dev):
        res = {"mean_cost": torch.empty(P, dtype=torch.float64, device=dev), "status": torch.empty(P, dtype=torch.int32, device=dev)}
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        check(lib.dt_sinkhorn_mean_cost(ptr(xa), a_ps, a_rs, n_a, ptr(xb), b_ps, b_rs, n_b, E, P, p, ptr(res["mean_cost"]),
                                        ptr(res["status"]), ptr(ws), ws_bytes, stream_ptr()), "dt_sinkhorn_mean_cost")
    return res


def _sinkhorn_epsilon(epsilon, P):
    """epsilon as given: a positive finite float (every state), or a float64 tensor [P] (checked on the device, per state)"""
    if isinstance(epsilon, torch.Tensor):
        if epsilon.dtype != torch.float64 or tuple(epsilon.shape) != (P,):
            raise ValueError(f"epsilon must be a float or a float64 tensor [{P}], got {epsilon.dtype} {tuple(epsilon.shape)}")
        return epsilon
    if isinstance(epsilon, bool) or not isinstance(epsilon, (int, float, np.integer, np.floating)):
        raise ValueError(f"epsilon={epsilon!r} must be a float or a float64 device tensor")
    if not (np.isfinite(epsilon) and epsilon > 0):
        raise ValueError(f"epsilon={epsilon!r} must be positive and finite")
    return float(epsilon)


def _sinkhorn_stop(max_iter, tol):
    max_iter = _count(max_iter, "max_iter", 1)
    if max_iter > SINKHORN_MAX_ITER:
        raise ValueError(f"max_iter={max_iter} is above {SINKHORN_MAX_ITER}")
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not (np.isfinite(tol) and tol >= 0):
        raise ValueError(f"tol={tol!r} must be a finite float >= 0")
    return max_iter, float(tol)


def device_sinkhorn_ot(a, b, epsilon, p=2, max_iter=SINKHORN_DEFAULT_MAX_ITER, tol=SINKHORN_DEFAULT_TOL, potentials=False,
                       workspace_bytes=None):
    """Entropic optimal-transport cost OT_eps between the sets of ``a`` and of ``b`` with uniform weights, state by state
    (dt_sinkhorn_ot): float32 device tensors [P, n, E] or [n, E] as ``device_swd`` takes them (n may differ between the
    sides; views are read in place; a side with one state is shared by all states of the other).  ``epsilon``: a float, or a
    float64 device tensor [P] (one per state, never brought to the host).  Sinkhorn steps on the dual potentials in the log
    domain with cost |a_i - b_j|^p; a state stops at the first step whose marginal error is <= ``tol`` (tol = 0: exactly
    ``max_iter`` steps).
    Returns device tensors {ot [P] float64, err [P] float64 (the marginal error of the last step run), iters [P] int32,
    status [P] int32 (bits: 1 a NaN or Inf in the state's rows, 2 an epsilon that is not finite or <= 0 -- ot and err are
    then NaN, iters 0 --, 4 not converged within max_iter: the values are still given)} and, with ``potentials``, f [P, n_a]
    and g [P, n_b].  ``workspace_bytes``: a cap on the scratch; the states then take turns, with the same bits.  There is
    no CPU fallback.  The contract is in include/dt_hip_sinkhorn.h."""
    p = _sinkhorn_p(p)
    max_iter, tol = _sinkhorn_stop(max_iter, tol)
    cap = None if workspace_bytes is None else _count(workspace_bytes, "workspace_bytes")
    sides, P = _sinkhorn_sides(a, b)
    epsilon = _sinkhorn_epsilon(epsilon, P)
    dev = _sinkhorn_devices(sides)
    if isinstance(epsilon, torch.Tensor):
        _on_device(epsilon, "epsilon")
        if epsilon.device != dev:
            raise ValueError(f"epsilon is on {epsilon.device}, the rows on {dev}")
        epsilon = epsilon.contiguous()
    (xa, _, n_a, E, a_ps, a_rs), (xb, _, n_b, _, b_ps, b_rs) = sides
    lib = _hip.load()
    ws_bytes = _sinkhorn_workspace(lib, P, n_a, n_b, cap)
    with torch.cuda.device(dev):
        eps = epsilon if isinstance(epsilon, torch.Tensor) else torch.full((P,), epsilon, dtype=torch.float64, device=dev)
        res = {"ot": torch.empty(P, dtype=torch.float64, device=dev), "err": torch.empty(P, dtype=torch.float64, device=dev),
               "iters": torch.empty(P, dtype=torch.int32, device=dev), "status": torch.empty(P, dtype=torch.int32, device=dev)}
        if potentials:
            res["f"] = torch.empty(P, n_a, dtype=torch.float64, device=dev)
            res["g"] = torch.empty(P, n_b, dtype=torch.float64, device=dev)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        check(lib.dt_sinkhorn_ot(ptr(xa), a_ps, a_rs, n_a, ptr(xb), b_ps, b_rs, n_b, E, P, p, ptr(eps), max_iter, tol,
                                 ptr(res["ot"]), ptr(res["err"]), ptr(res["iters"]), ptr(res["status"]),
                                 ptr(res["f"]) if potentials else None, ptr(res["g"]) if potentials else None, ptr(ws), ws_bytes,
                                 stream_ptr()), "dt_sinkhorn_ot")
    return res


def _sinkhorn_self(term, name, P, dev=None):
    """a self term handed in: the ``ot`` tensor (or the whole result) of an earlier ``device_sinkhorn_ot(x, x, ..)``"""
    ot = term["ot"] if isinstance(term, dict) and "ot" in term else term
    if not isinstance(ot, torch.Tensor) or ot.dtype != torch.float64 or ot.dim() != 1 or ot.shape[0] not in (1, P):
        raise ValueError(f"{name} must be the float64 ot tensor [{P}] (or [1]) of a self term")
    if dev is not None and ot.device != dev:
        raise ValueError(f"{name} is on {ot.device}, the rows on {dev}")
    return term if isinstance(term, dict) else {"ot": ot}


def device_sinkhorn_divergence(a, b, epsilon, p=2, max_iter=SINKHORN_DEFAULT_MAX_ITER, tol=SINKHORN_DEFAULT_TOL,
                               workspace_bytes=None, self_a=None, self_b=None):
    """Debiased Sinkhorn divergence S_eps(a, b) = OT_eps(a, b) - (0.5 OT_eps(a, a) + 0.5 OT_eps(b, b)), state by state:
    three ``device_sinkhorn_ot`` calls with one epsilon and that one float64 expression on the device.  All three terms go
    through the same kernels, so a ``b`` that is a bitwise copy of ``a`` gives exactly 0.0.  ``self_a`` / ``self_b``: a self term already made with the same
    epsilon, p, max_iter and tol: the whole result of its ``device_sinkhorn_ot`` call, whose err, iters and status then enter
    the ones returned here, or its bare ``ot`` tensor [P] (or [1] for a shared side), which CARRIES NO STATUS: err, iters
    and status then cover only the terms run in this call, and a NOT_CONVERGED bit of that self term is the caller's to
    keep.  A shape that does not fit is refused.  Returns device tensors {divergence, ot_ab, ot_aa,
    ot_bb [P] float64, err [P] (the largest of the three terms, but for one handed in as a bare tensor), iters [P] (likewise),
    status [P] (their bits OR-ed)}."""
    sides, P = _sinkhorn_sides(a, b)
    kw = dict(p=p, max_iter=max_iter, tol=tol, workspace_bytes=workspace_bytes)
    _sinkhorn_p(p), _sinkhorn_stop(max_iter, tol), _sinkhorn_epsilon(epsilon, P)
    if self_a is not None:
        self_a = _sinkhorn_self(self_a, "self_a", P)
    if self_b is not None:
        self_b = _sinkhorn_self(self_b, "self_b", P)
    dev = _sinkhorn_devices(sides)
    for term, name in ((self_a, "self_a"), (self_b, "self_b")):
        if term is not None:
            _sinkhorn_self(term, name, P, dev)

    def own(side, x):
        """the self term of a side; a shared side has one state, whose epsilon is the first (a float: the only one)"""
        if side[1] == 1 and P > 1 and isinstance(epsilon, torch.Tensor):
            raise ValueError("a side shared by several states needs one epsilon: hand its self term in (self_a / self_b)")
        return device_sinkhorn_ot(x, x, epsilon, **kw)

    raw = [_swd_rows(a, "a"), _swd_rows(b, "b")]
    ab = device_sinkhorn_ot(a, b, epsilon, **kw)
    aa = self_a if self_a is not None else own(raw[0], a)
    bb = self_b if self_b is not None else own(raw[1], b)
    ran = [t for t in (ab, aa, bb) if "status" in t]
    res = {"ot_ab": ab["ot"], "ot_aa": aa["ot"].expand(P), "ot_bb": bb["ot"].expand(P)}
    res["divergence"] = res["ot_ab"] - (0.5 * res["ot_aa"] + 0.5 * res["ot_bb"])
    res["err"] = torch.stack([t["err"].expand(P) for t in ran]).amax(dim=0)
    res["iters"] = torch.stack([t["iters"].expand(P) for t in ran]).amax(dim=0)
    status = ran[0]["status"].expand(P).clone()
    for t in ran[1:]:
        status |= t["status"].expand(P)
    res["status"] = status
    return res


# ---------------------------------------------------------------------- Fréchet distance (include/dt_hip_fid.h)
FID_MAX_SIDE = 2048
FID_MAX_ROWS = 32768
FID_EVENTS = 5


def _set_pair(a, b):
    """the two feature sets of device_fid / device_quality: float32, [n, D] or [P, n, D], one width, one problem count"""
    a, b = (_f32_rows(t, name, "[n, D] or [P, n, D]") for t, name in ((a, "a"), (b, "b")))
    if a.shape[-1] != b.shape[-1]:
        raise ValueError(f"b {tuple(b.shape)} does not match a {tuple(a.shape)}: both sets need the same feature width")
    if a.dim() == 3 and b.dim() == 3 and a.shape[0] != b.shape[0]:
        raise ValueError(f"b {tuple(b.shape)} does not match a {tuple(a.shape)}: the same number of problems, or one "
                         "2-D set shared by all of them")
    return a, b, a.shape[0] if a.dim() == 3 else (b.shape[0] if b.dim() == 3 else 1)


def _batch_limits(P, D):
    if not 1 <= P <= 65535:
        raise ValueError(f"unsupported number of problems P={P}")
    if D < 4 or D % 4 or D > (1 << 20):
        raise ValueError(f"the feature width must be a multiple of 4 in [4, 2^20], got D={D}")


def _fid_check(a, b):
    a, b, P = _set_pair(a, b)
    n_a, n_b, D = a.shape[-2], b.shape[-2], a.shape[-1]
    if n_a < 2 or n_b < 2:
        raise ValueError(f"a Fréchet distance needs at least 2 samples per set, got n_a={n_a}, n_b={n_b}")
    if min(n_a, n_b) > FID_MAX_SIDE or max(n_a, n_b) > FID_MAX_ROWS:
        raise ValueError(f"n_a={n_a}, n_b={n_b}: the device Fréchet distance takes min(n_a, n_b) <= {FID_MAX_SIDE} (and at "
                         f"most {FID_MAX_ROWS} per set); with more samples than that in both sets the rank is capped by "
                         "the feature width and the feature-space formula (calculate_fid on the host) is the right one")
    _batch_limits(P, D)
    return a, b, P


def _fid_rows(t):
    """(tensor, problem stride, row stride) as the kernel reads it: unit column stride, 16-byte aligned rows"""
    t = _aligned_rows(t)
    return t, (t.stride(0) if t.dim() == 3 else 0), t.stride(-2)


def device_fid(a, b, events=None, workspace=None):
    """Fréchet distance between the feature sets a and b, fp32 on the device: [n, D], or [P, n, D] for P problems; a 2-D
    set next to a 3-D one is shared by all P problems (one teacher against P students).  All arithmetic is fp64 on the
    device (dt_fid_distance): ``fid = |mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr sqrt(S_a S_b)`` with the last term from the
    singular values of the centred cross product, never a D x D matrix.  Returns device tensors {fid [P] fp64,
    parts [P, 4] fp64 = (|mu_a - mu_b|^2, tr S_a, tr S_b, tr sqrt(S_a S_b)), status [P] int32} (status: 0 ok, 1 a NaN or
    Inf in either set, the five doubles then NaN).  Limits: min(n_a, n_b) <= 2048, D % 4 == 0.  ``events``: None or 5
    torch.cuda.Event(enable_timing=True) recorded at the stage boundaries (dt_fid_distance).  ``workspace``: None (one is
    allocated) or a uint8 device tensor of at least ``dt_fid_workspace_bytes`` bytes; its contents do not matter."""
    a, b, P = _fid_check(a, b)
    return _fid_call(a, b, P, events, workspace, FID_EVENTS, "dt_fid_workspace_bytes", "dt_fid_distance")


def _set_pair_call(a, b, P, events, workspace, n_events, query, call, panel_rows=None):
    """The checked sets (a, b, P) through one set-pair entry of the library: the events count, the devices, the rows as the
    kernels read them, the workspace query ``query`` and the workspace.  ``panel_rows``: None, or ``lib -> rows`` for the
    entry whose query takes that fifth argument.  ``call(c)`` makes the entry call and returns what the caller returns;
    ``c`` holds ``lib``, ``dev``, ``rows`` (the entry's first ten arguments: a, n_a, its two strides, b, n_b, its two
    strides, P, D), ``panel_rows`` (the resolved value or None) and ``tail`` (its last four: workspace, its bytes, events,
    stream)."""
    if events is not None and len(events) != n_events:
        raise ValueError(f"events must be {n_events} torch.cuda.Event")
    _require_cuda(a, "a")
    _require_cuda(b, "b")
    if a.device != b.device:
        raise ValueError(f"a is on {a.device}, b on {b.device}")
    lib = _hip.load()
    n_a, n_b, D = a.shape[-2], b.shape[-2], a.shape[-1]
    (a, a_ps, a_rs), (b, b_ps, b_rs) = _fid_rows(a), _fid_rows(b)
    dev = a.device
    panel_rows = None if panel_rows is None else panel_rows(lib)
    ws_bytes = getattr(lib, query)(P, n_a, n_b, D, *(() if panel_rows is None else (panel_rows,)))
    if ws_bytes == 0:
        raise ValueError(f"{query} rejects P={P}, n_a={n_a}, n_b={n_b}, D={D}" +
                         ("" if panel_rows is None else f", panel_rows={panel_rows}"))
    with torch.cuda.device(dev):
        ev = _stage_events(events)
        ws = workspace
        if ws is None:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        elif ws.dtype != torch.uint8 or ws.device != dev or not ws.is_contiguous() or ws.numel() < ws_bytes:
            raise ValueError(f"workspace must be a contiguous uint8 tensor of >= {ws_bytes} bytes on {dev}")
        return call(types.SimpleNamespace(lib=lib, dev=dev, panel_rows=panel_rows,
                                          rows=(ptr(a), n_a, a_ps, a_rs, ptr(b), n_b, b_ps, b_rs, P, D),
                                          tail=(ptr(ws), ws_bytes, ev, stream_ptr())))


def _fid_call(a, b, P, events, workspace, n_events, query, entry):
    """the checked sets through one of the two Fréchet entries (they share the argument list)"""
    def call(c):
        out = {"fid": torch.empty(P, dtype=torch.float64, device=c.dev),
               "parts": torch.empty(P, 4, dtype=torch.float64, device=c.dev),
               "status": torch.empty(P, dtype=torch.int32, device=c.dev)}
        check(getattr(c.lib, entry)(*c.rows, ptr(out["fid"]), ptr(out["parts"]), ptr(out["status"]), *c.tail), entry)
        return out
    return _set_pair_call(a, b, P, events, workspace, n_events, query, call)


# ---------------------------------------------------------------------- the feature-space route (include/dt_hip_fid_cov.h)
FID_COV_MAX_ROWS = 131072
FID_COV_MAX_WIDTH = 2048
FID_COV_EVENTS = 7


def _fid_cov_check(a, b):
    a, b, P = _set_pair(a, b)
    n_a, n_b, D = a.shape[-2], b.shape[-2], a.shape[-1]
    if n_a < 2 or n_b < 2:
        raise ValueError(f"a Fréchet distance needs at least 2 samples per set, got n_a={n_a}, n_b={n_b}")
    _batch_limits(P, D)
    if max(n_a, n_b) > FID_COV_MAX_ROWS or D > FID_COV_MAX_WIDTH:
        raise ValueError(f"n_a={n_a}, n_b={n_b}, D={D}: the feature-space Fréchet distance on the device takes at most "
                         f"{FID_COV_MAX_ROWS} samples per set and a feature width of at most {FID_COV_MAX_WIDTH}")
    return a, b, P


def device_fid_cov(a, b, events=None, workspace=None):
    """``device_fid`` by the feature-space route (dt_fid_cov_distance): the same input forms and the same returned dict,
    for sets of up to 131072 rows each and a feature width of at most 2048.  The cross term comes from the singular
    values of ``L_a^T L_b``, with ``L`` the Cholesky factors of the two D x D centred covariance products (a pivot that is
    not above D 2^-52 max diag gives a zero column), all in fp64 on the device and every sum in a fixed order.  Sets
    shorter than D are legal, only slower than ``device_fid``; where both apply the two agree to rounding, not to the bit.
    ``events``: None or 7 torch.cuda.Event(enable_timing=True) (start, means + traces, covariances, factors, N and its
    square, tridiagonalisation, end).  ``workspace``: None or a uint8 device tensor of at least
    ``dt_fid_cov_workspace_bytes`` bytes; its contents do not matter."""
    a, b, P = _fid_cov_check(a, b)
    return _fid_call(a, b, P, events, workspace, FID_COV_EVENTS, "dt_fid_cov_workspace_bytes", "dt_fid_cov_distance")


def fid_route(n_a, n_b, D):
    """"samples" (``device_fid``: the smaller set has at most 2048 rows; every shape that route took before keeps it, and
    its bits) or "features" (``device_fid_cov``: both sets are longer than that and D <= 2048); ValueError if neither."""
    if min(n_a, n_b) <= FID_MAX_SIDE:
        return "samples"
    if D <= FID_COV_MAX_WIDTH:
        return "features"
    raise ValueError(f"n_a={n_a}, n_b={n_b}, D={D}: the device Fréchet distance takes min(n_a, n_b) <= {FID_MAX_SIDE} "
                     f"(the sample-space route) or a feature width D <= {FID_COV_MAX_WIDTH} (the feature-space route)")


def device_fid_auto(a, b, events=None, workspace=None):
    """``device_fid`` or ``device_fid_cov``, whichever ``fid_route`` names for the shapes of a and b (``events`` and
    ``workspace`` are that route's)."""
    a, b, _ = _set_pair(a, b)
    route = fid_route(a.shape[-2], b.shape[-2], a.shape[-1])
    return (device_fid if route == "samples" else device_fid_cov)(a, b, events=events, workspace=workspace)


# ---------------------------------------------------------------------- KID, precision / recall, density / coverage
# (include/dt_hip_quality.h)
QUALITY_MAX_ROWS = 2048
QUALITY_MAX_SUBSETS = 1024
QUALITY_EVENTS = 5


def _k_check(k, n_min, k_cap=None):
    """k, the neighbour count of both routes: an integer in [1, n_min - 1], and at most k_cap on the row-panel route"""
    k_max = n_min - 1
    top = k_max if k_cap is None else min(k_max, k_cap)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= top:
        raise ValueError(f"k={k!r} must be an integer in [1, min(n_a, n_b) - 1] = [1, {k_max}]" +
                         ("" if k_cap is None else f" and at most {k_cap} on the row-panel route"))


def _quality_check(a, b, k):
    a, b, P = _set_pair(a, b)
    for t, name in ((a, "a"), (b, "b")):
        if not 2 <= t.shape[-2] <= QUALITY_MAX_ROWS:
            raise ValueError(f"{name} holds {t.shape[-2]} rows: the device sample-quality scores take 2 .. "
                             f"{QUALITY_MAX_ROWS} per set")
    _batch_limits(P, a.shape[-1])
    _k_check(k, min(a.shape[-2], b.shape[-2]))
    return a, b, P


def _quality_subsets(subsets, n_a, n_b):
    """(idx_a, idx_b) -> two int32 host arrays [S, m], range and distinctness per row checked"""
    if not isinstance(subsets, (tuple, list)) or len(subsets) != 2:
        raise ValueError("subsets must be a pair (idx_a, idx_b) of integer tables [S, m]")
    tables = []
    for t, n, name in ((subsets[0], n_a, "subsets[0]"), (subsets[1], n_b, "subsets[1]")):
        t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        if t.ndim != 2 or not np.issubdtype(t.dtype, np.integer):
            raise ValueError(f"{name} must be an integer table [S, m], got shape {t.shape}, dtype {t.dtype}")
        if t.size and (t.min() < 0 or t.max() >= n):
            raise ValueError(f"{name} holds an index outside [0, {n})")
        s = np.sort(t, axis=1)
        if np.any(s[:, 1:] == s[:, :-1]):
            raise ValueError(f"{name} repeats an index within a row: the rows of a subset are distinct")
        tables.append(np.ascontiguousarray(t, dtype=np.int32))
    if tables[0].shape != tables[1].shape:
        raise ValueError(f"subsets[1] {tables[1].shape} does not match subsets[0] {tables[0].shape}")
    S, m = tables[0].shape
    if not 1 <= S <= QUALITY_MAX_SUBSETS or not 2 <= m <= min(n_a, n_b):
        raise ValueError(f"subsets: {S} subsets of size {m}; 1 .. {QUALITY_MAX_SUBSETS} subsets of size 2 .. "
                         f"min(n_a, n_b) = {min(n_a, n_b)}")
    return tables


def device_quality(a, b, k=5, subsets=None, radii=False, events=None, workspace=None):
    """KID, improved precision / recall and density / coverage between the feature sets a (the "real" set, the teacher) and
    b (the "generated" set, a student), fp32 on the device: [n, D], or [P, n, D] for P problems; a 2-D set next to a 3-D
    one is shared by all P problems.  All arithmetic is fp64 on the device (dt_quality_scores, whose header holds the
    definitions): the Gram matrices, the squared k-th nearest-neighbour radii (self included, as ``prdc`` counts),
    integer counts with strict ``<``, and the unbiased KID with the kernel ``(x.y / D + 1)^3``.  ``subsets``: None, or
    ``(idx_a, idx_b)`` int tables [S, m] of distinct row numbers per row; each gives one more KID, of those rows.
    Returns device tensors {kid [P] fp64, kid_subsets [P, S] fp64, counts [P, 4] int64 = (precision hits, recall hits,
    density pairs, coverage hits), precision, recall, density, coverage [P] fp64 = counts / (n_b, n_a, k n_b, n_a),
    status [P] int32 (0 ok, 1 a NaN or Inf in either set: the doubles are NaN, the counts -1)} and, with ``radii``,
    radii_a [P, n_a] and radii_b [P, n_b] fp64 (squared).  Limits: 2 .. 2048 rows per set, D % 4 == 0,
    1 <= k <= min(n_a, n_b) - 1.  ``events``: None or 5 torch.cuda.Event(enable_timing=True) recorded at the stage
    boundaries.  ``workspace``: None (one is allocated) or a uint8 device tensor of at least
    ``dt_quality_workspace_bytes`` bytes; its contents do not matter."""
    a, b, P = _quality_check(a, b, k)
    n_a, n_b, D = a.shape[-2], b.shape[-2], a.shape[-1]
    tables = None if subsets is None else _quality_subsets(subsets, n_a, n_b)
    S, m = (0, 0) if tables is None else tables[0].shape

    def call(c):
        kid, counts, status, r2 = _quality_outputs(P, S, n_a, n_b, radii, c.dev)
        sub = (None, None) if tables is None else tuple(torch.from_numpy(t).to(c.dev) for t in tables)
        check(c.lib.dt_quality_scores(*c.rows, int(k), ptr(sub[0]), ptr(sub[1]), S, m, ptr(kid), ptr(counts), ptr(r2),
                                      ptr(status), *c.tail), "dt_quality_scores")
        return _quality_result(kid, counts, status, r2, n_a, n_b, int(k))
    return _set_pair_call(a, b, P, events, workspace, QUALITY_EVENTS, "dt_quality_workspace_bytes", call)


def _quality_outputs(P, S, n_a, n_b, radii, dev):
    """(kid [P, 1 + S] fp64, counts [P, 4] int64, status [P] int32, squared radii [P, n_a + n_b] fp64 or None) for an
    entry to fill"""
    f64 = dict(dtype=torch.float64, device=dev)
    return (torch.empty(P, 1 + S, **f64), torch.empty(P, 4, dtype=torch.int64, device=dev),
            torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, n_a + n_b, **f64) if radii else None)


def _quality_result(kid, counts, status, r2, n_a, n_b, k):
    """the dict that device_quality and device_quality_stream return, from what their entries wrote"""
    c = counts.to(torch.float64)
    bad = counts[:, 0] < 0
    out = {"kid": kid[:, 0], "kid_subsets": kid[:, 1:], "counts": counts, "status": status}
    for name, col, den in (("precision", 0, n_b), ("recall", 1, n_a), ("density", 2, k * n_b), ("coverage", 3, n_a)):
        # a tensor divisor: torch divides by a Python scalar on the device as a product with its reciprocal
        out[name] = torch.where(bad, torch.full_like(c[:, col], float("nan")),
                                c[:, col] / torch.full_like(c[:, col], float(den)))
    if r2 is not None:
        out["radii_a"], out["radii_b"] = r2[:, :n_a], r2[:, n_a:]
    return out


# ---------------------------------------------------------------------- the same scores by row panels
# (include/dt_hip_quality_stream.h)
QUALITY_STREAM_MAX_ROWS = 131072
QUALITY_STREAM_MAX_K = 1023
QUALITY_STREAM_EVENTS = 6
QUALITY_STREAM_PANEL_ROWS = 1024          # the default panel, before it is cut to the rows and the workspace cap
QUALITY_STREAM_WORKSPACE_CAP = 2 << 30    # the default panel is lowered while the workspace would exceed this
QUALITY_SUBSET_CHUNK = 16                 # subsets per device_quality call of the panel route's subset KIDs


def _quality_stream_check(a, b, k, panel_rows):
    a, b, P = _set_pair(a, b)
    for t, name in ((a, "a"), (b, "b")):
        if not 2 <= t.shape[-2] <= QUALITY_STREAM_MAX_ROWS:
            raise ValueError(f"{name} holds {t.shape[-2]} rows: the row-panel route of the device sample-quality scores "
                             f"takes 2 .. {QUALITY_STREAM_MAX_ROWS} per set")
    _batch_limits(P, a.shape[-1])
    _k_check(k, min(a.shape[-2], b.shape[-2]), QUALITY_STREAM_MAX_K)
    if panel_rows is not None and (isinstance(panel_rows, bool) or not isinstance(panel_rows, (int, np.integer)) or
                                   not 64 <= panel_rows <= 4096 or panel_rows % 64):
        raise ValueError(f"panel_rows={panel_rows!r} must be None or a multiple of 64 in [64, 4096]")
    return a, b, P


def quality_stream_panel_rows(lib, P, n_a, n_b, D):
    """the default panel of ``device_quality_stream``: 1024 rows, cut to the rows there are (rounded up to 64), lowered in
    steps of 64 while ``dt_quality_stream_workspace_bytes`` exceeds 2 GiB"""
    rows = min(QUALITY_STREAM_PANEL_ROWS, (max(n_a, n_b) + 63) // 64 * 64)
    while rows > 64 and lib.dt_quality_stream_workspace_bytes(P, n_a, n_b, D, rows) > QUALITY_STREAM_WORKSPACE_CAP:
        rows -= 64
    return rows


def device_quality_stream(a, b, k=5, radii=False, panel_rows=None, events=None, workspace=None):
    """``device_quality`` by the row-panel route (dt_quality_stream_scores, whose header holds the method and the
    contract): the same input forms, the same definitions and the same returned dict (``kid_subsets`` is [P, 0]: this
    entry takes no subset tables), for sets of 2 .. 131072 rows each and k <= 1023.  No n x n matrix is held: the
    workspace is one panel of ``panel_rows`` rows of a Gram matrix per problem.  ``panel_rows``: None (1024, cut to the
    rows there are and lowered in steps of 64 while the workspace would exceed 2 GiB) or a multiple of 64 in 64 .. 4096;
    the outputs do not depend on it.  With a 2-D ``a`` next to a 3-D ``b`` the teacher's side is formed once.  Where both
    routes apply they agree to rounding (radii, KID), not to the bit.  ``events``: None or 6
    torch.cuda.Event(enable_timing=True) (start, diagonals and flags, the A side, the B side, the A x B panels, end).
    ``workspace``: None or a uint8 device tensor of at least ``dt_quality_stream_workspace_bytes`` bytes; its contents do
    not matter."""
    a, b, P = _quality_stream_check(a, b, k, panel_rows)
    n_a, n_b, D = a.shape[-2], b.shape[-2], a.shape[-1]

    def call(c):
        kid, counts, status, r2 = _quality_outputs(P, 0, n_a, n_b, radii, c.dev)
        check(c.lib.dt_quality_stream_scores(*c.rows, int(k), c.panel_rows, ptr(kid), ptr(counts), ptr(r2), ptr(status),
                                             *c.tail), "dt_quality_stream_scores")
        return _quality_result(kid, counts, status, r2, n_a, n_b, int(k))
    return _set_pair_call(
        a, b, P, events, workspace, QUALITY_STREAM_EVENTS, "dt_quality_stream_workspace_bytes", call,
        lambda lib: int(panel_rows) if panel_rows is not None else quality_stream_panel_rows(lib, P, n_a, n_b, D))


def quality_route(n_a, n_b, k):
    """"matrices" (``device_quality``: both sets have at most 2048 rows; every shape that route took before keeps it, and
    its bits) or "panels" (``device_quality_stream``: up to 131072 rows per set, k <= 1023); ValueError if neither."""
    if max(n_a, n_b) <= QUALITY_MAX_ROWS:
        return "matrices"
    if max(n_a, n_b) > QUALITY_STREAM_MAX_ROWS:
        raise ValueError(f"n_a={n_a}, n_b={n_b}: the device sample-quality scores take at most {QUALITY_MAX_ROWS} rows per "
                         f"set (whole Gram matrices) or at most {QUALITY_STREAM_MAX_ROWS} (row panels)")
    if k > QUALITY_STREAM_MAX_K:
        raise ValueError(f"k={k}: with more than {QUALITY_MAX_ROWS} rows in a set the device sample-quality scores go by "
                         f"row panels, which take k <= {QUALITY_STREAM_MAX_K}")
    return "panels"


def device_quality_auto(a, b, k=5, subsets=None, radii=False):
    """``device_quality`` or ``device_quality_stream``, whichever ``quality_route`` names for the shapes of a and b.  On
    the panel route ``subsets=(idx_a, idx_b)`` is served by gathering each subset's rows on the device into [S', m, D]
    tensors that go through ``device_quality(..., k=1)`` as problems of their own, at most 16 subsets per call; m <= 2048
    there."""
    a, b, P = _set_pair(a, b)
    n_a, n_b = a.shape[-2], b.shape[-2]
    if quality_route(n_a, n_b, k) == "matrices":
        return device_quality(a, b, k=k, subsets=subsets, radii=radii)
    if subsets is None:
        return device_quality_stream(a, b, k=k, radii=radii)
    ia, ib = _quality_subsets(subsets, n_a, n_b)
    if ia.shape[1] > QUALITY_MAX_ROWS:
        raise ValueError(f"subsets of size {ia.shape[1]}: with more than {QUALITY_MAX_ROWS} rows in a set a subset's KID is "
                         f"computed on its gathered rows, which takes subsets of at most {QUALITY_MAX_ROWS} rows")
    out = device_quality_stream(a, b, k=k, radii=radii)
    dev = out["kid"].device
    ia, ib = (torch.from_numpy(t).to(dev).long() for t in (ia, ib))
    cols = []
    for s0 in range(0, ia.shape[0], QUALITY_SUBSET_CHUNK):
        ca, cb = ia[s0:s0 + QUALITY_SUBSET_CHUNK], ib[s0:s0 + QUALITY_SUBSET_CHUNK]
        per_problem = []
        for p in range(P):
            rows_a, rows_b = (a[p] if a.dim() == 3 else a), (b[p] if b.dim() == 3 else b)
            per_problem.append(device_quality(rows_a[ca], rows_b[cb], k=1)["kid"])
        cols.append(torch.stack(per_problem))
    out["kid_subsets"] = torch.cat(cols, dim=1)
    return out


# ---------------------------------------------------------------------- perceptual distance (include/dt_hip_lpips.h)
def device_lpips(handle, images0, images1, in_scale=1.0, in_shift=0.0, per_layer=False):
    """LPIPS (v0.1, net='alex') between images0 [n0, 3, H, W] (n0 = 1: one image against all) and images1 [n1, 3, H, W]
    on ``handle`` (lpips.LPIPSHandle): two feature passes (dt_lpips_features) and one distance launch (dt_lpips_distance).
    ``in_scale * x + in_shift`` is applied first; (1, 0) takes images in [-1, 1] as they are.  Returns the device tensor
    [n1], with ``per_layer`` the pair ([n1], [n1, 5])."""
    from . import lpips
    lpips.check_images(images0)
    lpips.check_images(images1)
    if tuple(images0.shape[2:]) != tuple(images1.shape[2:]):
        raise ValueError(f"images0 {tuple(images0.shape)} and images1 {tuple(images1.shape)} differ in size")
    if images0.shape[0] not in (1, images1.shape[0]):
        raise ValueError(f"images0 holds {images0.shape[0]} images and images1 {images1.shape[0]}: one image, or as many")
    H, W = images1.shape[2:]
    p0 = handle.features(images0, in_scale, in_shift)
    p1 = handle.features(images1, in_scale, in_shift)
    return handle.distance(p0, p1, H, W, per_layer=per_layer)


def resize_bilinear(images, size):
    """``torch.nn.functional.interpolate(images, size=size, mode='bilinear', align_corners=True)`` for an NCHW fp32 tensor,
    on the device (dt_resize_bilinear); a host tensor is uploaded and the result stays on the device."""
    lib = _hip.load()
    if not images.is_cuda:
        if not torch.cuda.is_available():
            raise HipLibraryError("resize_bilinear needs a HIP device; there is no CPU fallback")
        images = images.to(torch.device("cuda", torch.cuda.current_device()))
    x = images.detach().contiguous().float()
    N, C, h, w = x.shape
    H, W = int(size[0]), int(size[1])
    out = torch.empty(N, C, H, W, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.dt_resize_bilinear(ptr(x), ptr(out), N * C, h, w, H, W, stream_ptr()), "dt_resize_bilinear")
    return out


def device_resampled_distance(longer, shorter):
    lib = _hip.load()
    nl, B, E = longer.shape
    ns = shorter.shape[0]
    out = torch.empty(B, ns, dtype=torch.float64, device=longer.device)
    with torch.cuda.device(longer.device):
        check(lib.dt_traj_resampled_distance(ptr(longer), ptr(shorter), nl, ns, B, E, ptr(out), stream_ptr()),
              "dt_traj_resampled_distance")
    return out


def metrics_from_sums(sums, w1, nT, nS, pixels, elems, resampled=None):
    """The 25-key dict of trajectory_metrics.py:12-325 from one pair's device reductions.

    sums: float64 [n_max,4] (dt_traj_metrics layout), w1: float64 [min(nT,nS)], resampled: float64
    [min] distances of the interp1d path (unequal lengths) or None.  The host part reproduces the
    reference's scalar arithmetic: fp32 where torch returned fp32 scalars, python floats elsewhere.
    """
    f32 = np.float32
    n = min(nT, nS)
    s32 = sums.astype(f32)                       # torch reduces in fp32 before .item()
    D = [float(np.sqrt(s32[i, 0])) for i in range(n)]
    Vt = [float(np.sqrt(s32[i, 1])) for i in range(1, nT)]
    Vs = [float(np.sqrt(s32[i, 2])) for i in range(1, nS)]
    m = {}
    # endpoint / final-image terms use each trajectory's OWN last state (row 0, slot 3)
    m["endpoint_distance"] = float(np.sqrt(s32[0, 3]))
    mse = float(s32[0, 3] / f32(elems))
    m["mse"] = mse
    acc = 0.0
    for i in range(n):
        acc += float(s32[i, 0] / f32(elems))
    m["trajectory_mse"] = np.log1p(1.0 - (acc / n) * 1000)
    m["point_by_point_similarity"] = np.exp(-5.0 * (np.mean(D) if D else float("inf")))
    m["log_mse_similarity"] = max(0, 1.0 - np.log1p(mse * 5000) / np.log1p(5000))
    tl = sl = 0
    for i in range(1, n):
        tl += Vt[i - 1] / pixels
        sl += Vs[i - 1] / pixels
    tl /= (n - 1)
    sl /= (n - 1)
    m["teacher_path_length"], m["student_path_length"] = tl, sl
    m["path_length_similarity"] = np.log1p(min(tl, sl) / max(tl, sl) if max(tl, sl) > 0 else 1.0)
    te = float(np.sqrt(s32[0, 1])) / tl if tl > 0 else 0
    se = float(np.sqrt(s32[0, 2])) / sl if sl > 0 else 0
    m["teacher_efficiency"], m["student_efficiency"] = te, se
    m["efficiency_similarity"] = np.log1p(min(te, se) / max(te, se) if max(te, se) > 0 else 1.0)
    m["teacher_velocities"], m["student_velocities"] = Vt, Vs
    vsim = [(min(a, b) / max(a, b) if max(a, b) > 0 else 1.0) for a, b in zip(Vt, Vs)]
    m["velocity_similarities"] = vsim
    m["mean_velocity_similarity"] = np.mean(vsim) if vsim else 0.0
    m["position_differences"] = list(D)
    m["mean_position_difference"] = np.mean(D) if D else 0.0
    m["max_position_difference"] = np.max(D) if D else 0.0
    cos, wcos = [], []
    for i in range(n - 1):
        vt, vs = f32(np.sqrt(s32[i + 1, 1])), f32(np.sqrt(s32[i + 1, 2]))
        if vt > 0 and vs > 0:
            c = float(s32[i + 1, 3] / (vt * vs))
            cos.append(c)
            wcos.append(c * ((float(vt) + float(vs)) / 2))
    m["directional_consistency"] = cos
    m["mean_directional_consistency"] = np.mean(cos) if cos else 0.0
    if wcos:
        total_w = sum((Vt[i] + Vs[i]) / 2 for i in range(min(len(Vt), len(Vs))))
        m["weighted_directional_consistency"] = (sum(wcos) / total_w if total_w > 0 else 0) ** 2
    else:
        m["weighted_directional_consistency"] = 0.0
    if resampled is None:
        pd = [f32(d) for d in D]                 # numpy norms of fp32 arrays stay fp32
    else:
        pd = [np.float64(d) for d in resampled]
    m["path_alignment"] = np.exp(-10.0 * np.sum(pd) / len(pd))
    W = [np.float64(v) for v in w1]
    m["wasserstein_distances"] = W
    m["mean_wasserstein"] = np.mean(W)
    m["distribution_similarity"] = np.log1p(np.exp(-m["mean_wasserstein"]))
    return m


SCALAR_KEYS = ("endpoint_distance", "mse", "trajectory_mse", "point_by_point_similarity", "log_mse_similarity",
               "teacher_path_length", "student_path_length", "path_length_similarity", "teacher_efficiency",
               "student_efficiency", "efficiency_similarity", "mean_velocity_similarity", "mean_position_difference",
               "max_position_difference", "mean_directional_consistency", "weighted_directional_consistency",
               "path_alignment", "mean_wasserstein", "distribution_similarity")


def batch_scalar_metrics(sums, w1, pixels, elems):
    """Vectorised form of ``metrics_from_sums`` for B equal-length pairs: {key: float64 array [B]} for the 19
    scalar metrics and ``trajectory_mse_pre`` (the per-step lists stay on the caller's side as sums / w1).

    sums float64 [B,n,4], w1 float64 [B,n].  Follows the same dtype path (fp32 where torch returned fp32
    scalars, float64 python arithmetic elsewhere, sequential accumulation where the reference loops)."""
    f32 = np.float32
    B, n, _ = sums.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        s32 = sums.astype(f32)
        D = np.sqrt(s32[:, :, 0]).astype(np.float64)              # [B,n]
        Vt = np.sqrt(s32[:, 1:, 1]).astype(np.float64)            # [B,n-1]
        Vs = np.sqrt(s32[:, 1:, 2]).astype(np.float64)
        out = {}
        out["endpoint_distance"] = np.sqrt(s32[:, 0, 3]).astype(np.float64)
        mse = (s32[:, 0, 3] / f32(elems)).astype(np.float64)
        out["mse"] = mse
        step_mse = (s32[:, :, 0] / f32(elems)).astype(np.float64)
        acc = np.zeros(B)
        for i in range(n):
            acc = acc + step_mse[:, i]
        # 1000 x mean step-MSE, before the reference's log1p(1 - x), which is NaN for x > 2: finite, and the value to compare
        out["trajectory_mse_pre"] = (acc / n) * 1000
        out["trajectory_mse"] = np.log1p(1.0 - out["trajectory_mse_pre"])
        meanD = D.mean(axis=1)
        out["point_by_point_similarity"] = np.exp(-5.0 * meanD)
        lms = 1.0 - np.log1p(mse * 5000) / np.log1p(5000)
        out["log_mse_similarity"] = np.where(lms > 0, lms, 0.0)      # python max(0, x): NaN -> 0
        tl, sl = np.zeros(B), np.zeros(B)
        for i in range(n - 1):
            tl = tl + Vt[:, i] / pixels
            sl = sl + Vs[:, i] / pixels
        tl, sl = tl / (n - 1), sl / (n - 1)
        out["teacher_path_length"], out["student_path_length"] = tl, sl
        hi = np.maximum(tl, sl)
        out["path_length_similarity"] = np.log1p(np.where(hi > 0, np.minimum(tl, sl) / np.where(hi > 0, hi, 1), 1.0))
        te = np.where(tl > 0, np.sqrt(s32[:, 0, 1]).astype(np.float64) / np.where(tl > 0, tl, 1), 0.0)
        se = np.where(sl > 0, np.sqrt(s32[:, 0, 2]).astype(np.float64) / np.where(sl > 0, sl, 1), 0.0)
        out["teacher_efficiency"], out["student_efficiency"] = te, se
        hi = np.maximum(te, se)
        out["efficiency_similarity"] = np.log1p(np.where(hi > 0, np.minimum(te, se) / np.where(hi > 0, hi, 1), 1.0))
        vhi = np.maximum(Vt, Vs)
        vsim = np.where(vhi > 0, np.minimum(Vt, Vs) / np.where(vhi > 0, vhi, 1), 1.0)
        out["mean_velocity_similarity"] = vsim.mean(axis=1) if n > 1 else np.zeros(B)
        out["mean_position_difference"] = meanD
        out["max_position_difference"] = D.max(axis=1)
        vt32, vs32 = np.sqrt(s32[:, 1:, 1]), np.sqrt(s32[:, 1:, 2])
        ok = (vt32 > 0) & (vs32 > 0)
        cos = np.where(ok, (s32[:, 1:, 3] / np.where(ok, vt32 * vs32, f32(1))).astype(np.float64), 0.0)
        cnt = ok.sum(axis=1)
        csum = np.zeros(B)
        wsum = np.zeros(B)
        for i in range(n - 1):
            csum = csum + cos[:, i]
            wsum = wsum + cos[:, i] * ((Vt[:, i] + Vs[:, i]) / 2) * ok[:, i]
        out["mean_directional_consistency"] = np.where(cnt > 0, csum / np.where(cnt > 0, cnt, 1), 0.0)
        tw = np.zeros(B)
        for i in range(n - 1):
            tw = tw + (Vt[:, i] + Vs[:, i]) / 2
        out["weighted_directional_consistency"] = np.where(cnt > 0, np.where(tw > 0, wsum / np.where(tw > 0, tw, 1), 0.0) ** 2, 0.0)
        pd32 = np.sqrt(s32[:, :, 0])                                # numpy norms of fp32 arrays stay fp32
        out["path_alignment"] = np.exp(-10.0 * pd32.sum(axis=1, dtype=f32) / n).astype(np.float64)
        mw = w1.mean(axis=1)
        out["mean_wasserstein"] = mw
        out["distribution_similarity"] = np.log1p(np.exp(-mw))
    return out
