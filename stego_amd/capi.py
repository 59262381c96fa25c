"""ctypes binding of libstego_corr.so (include/*.h) for torch tensors: the calls.  stego_amd._abi declares the ABI (structures,
constants, SIGNATURES) and is re-exported here.

This is the ONLY compute backend of stego_amd: there is no PyTorch/CPU fallback.  If the
library is missing or the tensors are not on a HIP device the calls raise.
PyTorch is used for device memory (caching allocator), streams and autograd plumbing only.

How a call reaches the library:
  * _call(name, *args) coerces each argument by the type SIGNATURES gives it.  The one-liners are built on it: NAME_raw =
    _raw("stego_NAME") hands a launching export out as it is, return code unchecked (tests: the error codes), and the wrappers
    that take tensors (crf_loss, kmeans_step, ...) check their arguments, allocate and _check() that raw call; _launch_plan,
    adam_plan, step_stats_plan and aug_check_params use it for their host tables;
  * NAME_workspace_bytes = _bytes(...) and NAME_desc = _desc(StegoNameDesc) are one-liners of their own helpers;
  * the per-step wrappers (corr_fwd / corr_bwd, helper_*, head_*, the draws, step_stats_call) and the older wrappers written
    before _call (the CRF, the data store, sample / dense_corr / knn, the *_plan readers with out-parameters) call lib.stego_*
    directly with byref() and _ptr().
A new unit adds its structure, constants and signatures to _abi.py, and here one _raw / _bytes / _desc line per export and the wrapper.
"""
import ctypes
import os
from ctypes import Structure, byref, c_float, c_int32, c_int64, c_size_t, c_void_p

import torch

from . import _build
from ._abi import *  # noqa: F401,F403
from ._abi import _D, _H, _M, _P, _V  # noqa: F401

RENDER_DTYPES = {torch.int64: RENDER_I64, torch.int32: RENDER_I32, torch.uint8: RENDER_U8}
REGIONS_DTYPES = {torch.int64: REGIONS_I64, torch.int32: REGIONS_I32, torch.uint8: REGIONS_U8}

_lib = None


def library_path():
    """The in-tree library - or the file STEGO_LIB_PATH names (the sanitizer build of tests/test_asan_host.py; tools)."""
    return os.environ.get("STEGO_LIB_PATH") or _build.LIB_PATH


def load():
    """dlopen the in-tree library (never builds implicitly on a GPU box: build() is explicit)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            "stego_amd: %s is missing - the HIP extension is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc); there is no fallback path." % path)
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)     # AttributeError if the .so is stale / symbol missing
        fn.restype = res
        fn.argtypes = args
        _CALLS[name] = (fn, len(args), tuple((i, c) for i, c in enumerate(map(_converter, args)) if c is not None))
    if lib.stego_abi_version() != ABI_VERSION:
        raise RuntimeError("stego_amd: ABI version mismatch, rebuild the library")
    _lib = lib
    return lib


KNOBS = {"STEGO_DEBUG": 0, "STEGO_DEBUG_SAMPLE": 1, "STEGO_DEBUG_BWD": 2, "STEGO_DEBUG_VIT": 3, "STEGO_DEBUG_KNN": 4,
         "STEGO_FWD_VARIANT": 5, "STEGO_SHARED_DEVICE": 6}


_shared_device_default = False


def set_shared_device(shared=True):
    """Default of the per-call flag STEGO_FLAG_SHARED_DEVICE for descriptors made by make_desc() from now on: other kernels
    (collectives) run on the device beside the loss, so the fused forward launches one workgroup per tile instead of one per
    compute unit (include/stego_corr.h).  A per-call property of the descriptor since ABI 3 - nothing in the library is global;
    `cfg.shared_device` (ContrastiveCorrelationLoss) or make_desc(..., shared_device=...) override this default."""
    global _shared_device_default
    _shared_device_default = bool(shared)


def debug_set(name, value):
    """Measurement knob of the library (tools only; the library reads the environment once, at load)."""
    _check(load().stego_debug_set(KNOBS[name], int(value)))


def _check(rc):
    if rc != 0:
        _WS_CACHE.clear()            # a kept workspace may hold dirty hand-off words after a failed launch
        _WS_PINNED.clear()
        if _torchglue_mod:           # ... and so may the ones the C++ autograd function keeps
            _torchglue_mod.reset_workspaces()
        msg = load().stego_error_string(rc).decode()
        raise RuntimeError("libstego_corr error %d: %s" % (rc, msg))


def _require_dev(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("stego_amd runs on MI355X only: got a %s tensor (no CPU fallback exists)" % t.device)


def _map(t):
    if t.dtype != torch.float32 or t.dim() != 4:
        raise RuntimeError("expected a float32 [N,C,H,W] tensor, got %s %s" % (t.dtype, tuple(t.shape)))
    s = t.stride()
    return StegoMap(t.data_ptr(), s[0], s[1], s[2], s[3])


def _ptr(t):
    return None if t is None else t.data_ptr()


def _addr(x):
    """What a void* argument takes: a tensor's address, a structure's address; a raw address or None as it is (tests hand the *_raw
    functions NULL and misaligned pointers), and so a ctypes array (a host table), whose address ctypes passes itself."""
    if x is None:
        return x
    if torch.is_tensor(x):
        return x.data_ptr()
    return ctypes.addressof(x) if isinstance(x, Structure) else x


def _converter(ctype):
    """What _call does to an argument that SIGNATURES declares as `ctype`; None: nothing."""
    if ctype is c_void_p:
        return _addr
    if issubclass(ctype, ctypes._Pointer):
        # POINTER(StegoX): ctypes itself passes a StegoX instance by reference and None as NULL; out-parameters and arrays
        # (POINTER(c_int32), ...) go as given
        return None
    return float if ctype in (c_float, ctypes.c_double) else int


_CALLS = {}     # export -> (the C function, its argument count, ((position, converter) of every argument that has one)), filled by load()


def _call(name, *args):
    """The export `name` on arguments as Python has them: a structure or None where it takes one by reference, a tensor, a ctypes
    array, an address or None where it takes a pointer, numbers as they come.  -> the return code (or byte count) as an int,
    unchecked."""
    if _lib is None:
        load()
    fn, n, convert = _CALLS[name]
    if len(args) != n:
        raise TypeError("%s takes %d arguments, got %d" % (name, n, len(args)))
    args = list(args)
    for i, c in convert:
        if args[i].__class__ is not int:        # (ctypes takes an int as it is for every scalar and pointer type: most arguments)
            args[i] = c(args[i])
    return int(fn(*args))


def _raw(name):
    """NAME_raw = _raw("stego_NAME"), for an export whose last parameter is the stream: the export with every argument given, in the
    header's order (maps as StegoMap or None, the rest tensors, raw addresses or None; `stream` last, by name, or left out: NULL) ->
    the return code, unchecked."""
    n = len(SIGNATURES[name][1])

    def raw(*args, stream=None):
        return _call(name, *args, stream) if len(args) == n - 1 else _call(name, *args)
    return raw


def _bytes(name):
    """NAME_workspace_bytes = _bytes("stego_NAME_workspace_bytes") (host only) -> the bytes; 0 for an invalid descriptor."""
    def workspace_bytes(desc):
        return int(getattr(_lib or load(), name)(desc))
    return workspace_bytes


def _desc(cls, **defaults):
    """NAME_desc = _desc(StegoNameDesc, flags=0): a descriptor from its fields in the structure's order, by position or by name, each
    coerced to its C type (int / float); `defaults` for trailing fields."""
    names = tuple(n for n, _ in cls._fields_)
    coerce = tuple(float if t in (c_float, ctypes.c_double) else int for _, t in cls._fields_)

    def make(*args, **kw):
        if not kw and len(args) == len(names):
            try:
                return cls(*args)       # every value already of its field's kind (the per-step callers): ctypes takes them as they are
            except TypeError:           # e.g. a float for an integer field: coerced below, as int() does
                pass
        else:
            given = dict(defaults, **dict(zip(names, args)), **kw)      # (a field given twice is dict()'s TypeError)
            if len(args) > len(names) or set(given) != set(names):
                raise TypeError("%s takes (%s), got %d values and %s" % (cls.__name__, ", ".join(names), len(args), sorted(kw)))
            args = [given[k] for k in names]
        return cls(*[c(a) for c, a in zip(coerce, args)])
    return make


def _workspace_need(workspace_bytes, desc, reject):
    """The workspace bytes `desc` needs, from the unit's NAME_workspace_bytes.  0 bytes = an invalid descriptor: reject() - the unit's
    host-only plan where it has one, else the entry point without buffers - names the error and _check raises it before any output
    is sized from the descriptor."""
    need = workspace_bytes(desc)
    if need == 0:
        _check(reject())
    return need


def _workspace(workspace_bytes, desc, dev, reject):
    """(a fresh workspace tensor, its bytes) for `desc`; an invalid descriptor raises as in _workspace_need."""
    need = _workspace_need(workspace_bytes, desc, reject)
    return _empty_bytes(need, dev), need


def _expect(who, name, t, dtype, shape):
    """Raise unless `t` is a contiguous tensor of this dtype and shape (None: any extent)."""
    if t.dtype != dtype or t.dim() != len(shape) or not t.is_contiguous() or any(s is not None and s != n for s, n in zip(shape, t.shape)):
        raise RuntimeError("%s: %s must be a contiguous %s tensor of shape %s, got %s %s"
                           % (who, name, dtype, tuple(shape), t.dtype, tuple(t.shape)))


def _launch_plan(name, desc, n):
    """An array-style stego_*_plan export (host only) -> (return code, [(LDS bytes, workgroups) of each of the n launches])."""
    lds, wgs = (c_size_t * n)(), (c_int64 * n)()
    rc = _call(name, desc, lds, wgs)
    return rc, [(int(a), int(b)) for a, b in zip(lds, wgs)]


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """hipStream_t of torch's current stream on the current device (the raw accessor: torch.cuda.current_stream() costs ~10 us of
    Python per call, three calls per training step)."""
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


class _on_device:
    """`with torch.cuda.device(dev)` only when dev is not already current (the context manager is ~8 us of Python)."""
    __slots__ = ("guard",)

    def __init__(self, dev):
        idx = dev.index if dev.index is not None else 0
        self.guard = None if (_raw_device is not None and _raw_device() == idx) else torch.cuda.device(dev)

    def __enter__(self):
        if self.guard is not None:
            self.guard.__enter__()

    def __exit__(self, *exc):
        if self.guard is not None:
            return self.guard.__exit__(*exc)
        return False


def make_desc(B, C, K, H, W, S, n_neg, cfg, shifts, precision=PREC_F32, shared_device=None):
    if shared_device is None:
        shared_device = getattr(cfg, "shared_device", None)
    if shared_device is None:
        shared_device = _shared_device_default
    return StegoCorrDesc(B, C, K, H, W, S, n_neg, int(bool(cfg.pointwise)), int(bool(cfg.zero_clamp)),
                         int(bool(cfg.stabalize)), float(shifts[0]), float(shifts[1]), float(shifts[2]),
                         int(precision), FLAG_SHARED_DEVICE if shared_device else 0)


def occupy(n_workgroups, lds_bytes=64 * 1024, microseconds=80, stream=None):
    """Test hook (stego_debug_occupy): a stand-in for a foreign kernel holding compute units while the loss runs."""
    _check(load().stego_debug_occupy(int(n_workgroups), int(lds_bytes), int(microseconds),
                                     stream.cuda_stream if stream is not None else _stream()))


def _dense(t, dtype):
    if t.dtype != dtype:
        t = t.to(dtype)
    return t if t.is_contiguous() else t.contiguous()


def _empty_bytes(n, dev):
    return torch.empty(max(int(n), 16), dtype=torch.uint8, device=dev)


# Forward workspaces are kept (per device, stream and descriptor): the fused forward hands data between workgroups through
# a few counters in the workspace that must be zero when a launch starts and that every launch leaves zero again.  A kept
# workspace is prepared once (stego_corr_workspace_prepare) and then costs neither an allocation nor a memset per call.
_WS_CACHE = {}
_WS_PINNED = set()        # keys of workspaces first used during a stream capture
_SIDE_READY = set()
_WS_CACHE_MAX = 16


def reset_workspaces():
    """Forget the kept forward workspaces (call after a launch that failed: its counters may be dirty)."""
    _WS_CACHE.clear()
    _WS_PINNED.clear()
    if _torchglue_mod:
        _torchglue_mod.reset_workspaces()


def _prepared_ws(lib, desc, dev):
    n = int(lib.stego_corr_workspace_bytes(byref(desc)))
    stream = _stream()
    key = (dev.index, int(stream or 0), n, bytes(desc))
    ws = _WS_CACHE.get(key)
    if ws is None:
        if len(_WS_CACHE) >= _WS_CACHE_MAX:
            # forget the oldest workspace that no captured graph holds (a graph replays with the pointer it captured: its workspace
            # must live as long as this cache does)
            for k in _WS_CACHE:
                if k not in _WS_PINNED:
                    _WS_CACHE.pop(k)
                    break
        ws = _empty_bytes(n, dev)
        with _on_device(dev):
            if torch.cuda.is_current_stream_capturing():
                _WS_PINNED.add(key)
                # a workspace first met while a graph is being captured (the capture stream is a stream of its own): prepared NOW on
                # the library's side stream, not as a memset node that every replay would repeat in front of the forward (launches
                # leave their counters zero, so once is enough)
                _check(lib.stego_corr_workspace_prepare_now(byref(desc), _ptr(ws), ws.numel()))
            else:
                _check(lib.stego_corr_workspace_prepare(byref(desc), _ptr(ws), ws.numel(), stream))
                if dev.index not in _SIDE_READY:       # the library's side stream for this device: created outside any capture
                    _check(lib.stego_corr_workspace_prepare_now(None, None, 0))
                    _SIDE_READY.add(dev.index)
        _WS_CACHE[key] = ws
    return ws


def _fwd_buffers(lib, desc, dev, need_grad, flat=False, keep_ws=False):
    B, S, n_neg = desc.B, desc.S, desc.n_neg
    f32 = dict(dtype=torch.float32, device=dev)
    shp = (S ** 4,) if flat else (S, S, S, S)
    loss_means = torch.empty(3, **f32)
    intra_cd = torch.empty(B, *shp, **f32)
    inter_cd = torch.empty(B, *shp, **f32)
    neg_loss = torch.empty(n_neg * B, *shp, **f32)
    neg_cd = torch.empty(n_neg * B, *shp, **f32)
    saved_w = torch.empty((2 + n_neg) * B, S ** 4, **f32) if need_grad else None
    saved_mean = torch.empty(2 + n_neg, **f32) if need_grad else None
    saved_ctx = _empty_bytes(lib.stego_corr_saved_ctx_bytes(byref(desc)), dev) if need_grad else None
    ws = _prepared_ws(lib, desc, dev) if keep_ws else _empty_bytes(lib.stego_corr_workspace_bytes(byref(desc)), dev)
    return loss_means, intra_cd, inter_cd, neg_loss, neg_cd, saved_w, saved_mean, saved_ctx, ws


def corr_fwd(desc, feats, feats_pos, code, code_pos, coords1, coords2, perms, need_grad):
    """stego_corr_fwd on torch tensors. Returns (loss_means[3], intra_cd, inter_cd, neg_loss, neg_cd,
    saved) where saved = (saved_w, saved_mean, saved_ctx) or None."""
    _require_dev(feats, feats_pos, code, code_pos, coords1, coords2, perms)
    lib = load()
    dev = feats.device
    coords1 = _dense(coords1, torch.float32)
    coords2 = _dense(coords2, torch.float32)
    perms = _dense(perms, torch.int64) if desc.n_neg else None
    (loss_means, intra_cd, inter_cd, neg_loss, neg_cd, saved_w, saved_mean, saved_ctx, ws) = _fwd_buffers(
        lib, desc, dev, need_grad, keep_ws=True)
    mf, mfp, mc, mcp = _map(feats), _map(feats_pos), _map(code), _map(code_pos)
    with _on_device(dev):
        _check(lib.stego_corr_fwd_prepared(byref(desc), byref(mf), byref(mfp), byref(mc), byref(mcp),
                                  _ptr(coords1), _ptr(coords2), _ptr(perms),
                                  _ptr(loss_means), _ptr(intra_cd), _ptr(inter_cd), _ptr(neg_loss), _ptr(neg_cd),
                                  _ptr(saved_w), _ptr(saved_mean), _ptr(saved_ctx), _ptr(ws), ws.numel(), _stream()))
    saved = (saved_w, saved_mean, saved_ctx) if need_grad else None
    return loss_means, intra_cd, inter_cd, neg_loss, neg_cd, saved


def finish_draws(u1, u2, raw_perms, B):
    """(coords1, coords2, perms) from torch.rand x2 and the n_neg torch.randperm results, one launch (stego_finish_draws)."""
    lib = load()
    dev = u1.device
    n_neg = len(raw_perms)
    c1 = torch.empty_like(u1)
    c2 = torch.empty_like(u2)
    perms = torch.empty(n_neg, B, dtype=torch.int64, device=dev)
    arr = (ctypes.c_void_p * max(n_neg, 1))(*[r.data_ptr() for r in raw_perms])
    with _on_device(dev):
        _check(lib.stego_finish_draws(_ptr(u1), _ptr(u2), u1.numel(), arr, n_neg, B, _ptr(c1), _ptr(c2), _ptr(perms), _stream()))
    return c1, c2, perms


_torchglue_mod = None


def torchglue():
    """The in-tree torch extension (csrc/torch_glue_ext.cpp): the loss as a C++ autograd function over the C ABI and the device
    generator's graph-safe Philox state - or None when it has not been built (then the Python autograd.Function runs, and draws under
    stream capture stay the torch calls)."""
    global _torchglue_mod
    if _torchglue_mod is None:
        path = _build.TORCHGLUE_PATH
        if not os.path.exists(path):
            _torchglue_mod = False
        else:
            import importlib.util
            load()
            try:
                spec = importlib.util.spec_from_file_location("_stego_torchglue", path)
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                mod.bind(library_path())      # (the SAME file ctypes loaded: with STEGO_LIB_PATH set two copies would each own their globals - ADVICE round 5)
                _torchglue_mod = mod
            except (ImportError, OSError, RuntimeError) as e:      # e.g. a stale build against another torch: the product runs without it
                import warnings
                warnings.warn("stego_amd: %s does not load (%s: %s) - using the Python autograd function; rebuild with "
                              "stego_amd._build.build_torchglue(force=True)" % (path, type(e).__name__, str(e)[:200]))
                _torchglue_mod = False
    return _torchglue_mod or None


_ADVANCE = {}


def ref_draws(gen, shape, n_neg, B, variant, dev):
    """(coords1, coords2, perms) = the reference's torch.rand x 2 / torch.randperm x n_neg draws from ONE launch (stego_ref_draws),
    bit for bit, advancing `gen` (the device's torch.Generator) exactly as the torch calls would.  While the current stream is being
    captured the kernel reads the generator's state where CUDAGraph.replay puts it (stego_ref_draws_indirect; needs torchglue())."""
    ext = torchglue()
    if ext is not None and len(shape) == 4 and shape[1] == shape[2] and shape[3] == 2 and shape[0] == B:
        return ext.ref_draws(gen, B, shape[1], n_neg, variant, dev)
    lib = load()
    c1 = torch.empty(shape, dtype=torch.float32, device=dev)
    c2 = torch.empty(shape, dtype=torch.float32, device=dev)
    perms = torch.empty(n_neg, B, dtype=torch.int64, device=dev)
    with _on_device(dev):
        adv = int(lib.stego_ref_draws_advance(c1.numel(), n_neg, B, variant))
        if ext is not None:
            captured, seed, off, intra = ext.philox_state(gen, adv)
            if captured:
                _check(lib.stego_ref_draws_indirect(seed, off, intra, variant, c1.numel(), n_neg, B, _ptr(c1), _ptr(c2), _ptr(perms), _stream()))
            else:
                _check(lib.stego_ref_draws(seed, off, variant, c1.numel(), n_neg, B, _ptr(c1), _ptr(c2), _ptr(perms), _stream()))
            return c1, c2, perms
        seed, off = gen.initial_seed(), gen.get_offset()
        _check(lib.stego_ref_draws(seed & (2 ** 64 - 1), off, variant, c1.numel(), n_neg, B, _ptr(c1), _ptr(c2), _ptr(perms), _stream()))
    gen.set_offset(off + adv)
    return c1, c2, perms


def ref_dropout_masks(gen, n_masks, numel, keep_prob, variant, dev):
    """n_masks x `x.new_empty(B, C, 1, 1).bernoulli_(keep_prob).div_(keep_prob)` (what nn.Dropout2d draws per call) from ONE launch,
    bit for bit, advancing `gen` like the torch calls -> float32 [n_masks, numel].  Needs torchglue() (the generator's Philox state)."""
    lib = load()
    ext = torchglue()
    if ext is None:
        raise RuntimeError("ref_dropout_masks needs the torch glue extension")
    out = torch.empty(n_masks, numel, dtype=torch.float32, device=dev)
    with _on_device(dev):
        adv = int(lib.stego_ref_dropout_masks_advance(numel, n_masks, variant))
        captured, seed, off, intra = ext.philox_state(gen, adv)
        if captured:
            _check(lib.stego_ref_dropout_masks(0, intra, seed, off, variant, n_masks, numel, float(keep_prob), _ptr(out), _stream()))
        else:
            _check(lib.stego_ref_dropout_masks(seed, off, None, None, variant, n_masks, numel, float(keep_prob), _ptr(out), _stream()))
    return out


def fast_draws(seed, shape, n_neg, B):
    """(coords1, coords2, perms) of the reference's distributions from ONE launch (stego_fast_draws); `seed`: int64 [1] on the
    device, drawn by the caller from the torch generator.  Not the reference's random stream (cfg.fast_draws)."""
    lib = load()
    dev = seed.device
    c1 = torch.empty(shape, dtype=torch.float32, device=dev)
    c2 = torch.empty(shape, dtype=torch.float32, device=dev)
    perms = torch.empty(n_neg, B, dtype=torch.int64, device=dev)
    with _on_device(dev):
        _check(lib.stego_fast_draws(_ptr(seed), c1.numel(), n_neg, B, _ptr(c1), _ptr(c2), _ptr(perms), _stream()))
    return c1, c2, perms


def event_counters(desc, ws):
    """(tiles that gave up waiting for their anchor, negative tiles whose old_mean rendezvous timed out) since the forward workspace `ws`
    was prepared (stego_corr_event_counters: two device words; this copies them - a synchronisation, tools and tests only)."""
    lib = load()
    p = lib.stego_corr_event_counters(byref(desc), _ptr(ws), ws.numel())
    if not p:
        raise RuntimeError("stego_corr_event_counters: bad descriptor or workspace")
    off = int(p) - ws.data_ptr()
    w = ws[off: off + 8].view(torch.int32).cpu()
    return int(w[0]), int(w[1])


def event_counters_total():
    """Sum of event_counters() over every forward workspace this process keeps (the Python wrapper's and the C++ autograd function's):
    (tiles that sampled their anchor themselves, old_mean rendezvous that timed out) since those workspaces were prepared.  Both are zero
    in normal operation; non-zero = the single-launch forward keeps taking its fallback paths (device shared or partitioned without
    cfg.shared_device / STEGO_FLAG_SHARED_DEVICE): correct, ~30 us slower per step.  A synchronisation: call it every few hundred steps."""
    g = r = 0
    seen = []
    for key, ws in list(_WS_CACHE.items()):
        seen.append((key[3], ws))
    mod = torchglue()
    if mod is not None and hasattr(mod, "workspaces"):
        seen += list(mod.workspaces())
    for dbytes, ws in seen:
        desc = StegoCorrDesc.from_buffer_copy(dbytes)
        if desc.S * desc.S > 128:                   # the multi-launch path (csrc/corr_wide.hip) has no hand-off words
            continue
        a, b = event_counters(desc, ws)
        g += a
        r += b
    return g, r


def corr_fwd_launches(desc, feats, feats_pos, code, code_pos):
    """Kernel launches stego_corr_fwd_prepared needs for these maps: 1 = the fused forward, 3 = sample / tile / finalize."""
    lib = load()
    mf, mfp, mc, mcp = _map(feats), _map(feats_pos), _map(code), _map(code_pos)
    return int(lib.stego_corr_fwd_launches(byref(desc), byref(mf), byref(mfp), byref(mc), byref(mcp)))


def corr_fwd_profile(desc, feats, feats_pos, code, code_pos, coords1, coords2, perms, need_grad, iters):
    """stego_corr_fwd_profile: mean HIP-event duration (ms) of (sample kernel, tile kernel, finalize kernel)."""
    _require_dev(feats, feats_pos, code, code_pos, coords1, coords2, perms)
    lib = load()
    dev = feats.device
    (loss_means, intra_cd, inter_cd, neg_loss, neg_cd, saved_w, saved_mean, saved_ctx, ws) = _fwd_buffers(
        lib, desc, dev, need_grad, flat=True)
    mf, mfp, mc, mcp = _map(feats), _map(feats_pos), _map(code), _map(code_pos)
    ms = (c_float * 3)()
    with _on_device(dev):
        _check(lib.stego_corr_fwd_profile(byref(desc), byref(mf), byref(mfp), byref(mc), byref(mcp),
                                          _ptr(coords1), _ptr(coords2), _ptr(perms) if desc.n_neg else None,
                                          _ptr(loss_means), _ptr(intra_cd), _ptr(inter_cd), _ptr(neg_loss),
                                          _ptr(neg_cd), _ptr(saved_w), _ptr(saved_mean), _ptr(saved_ctx),
                                          _ptr(ws), ws.numel(), _stream(), int(iters), ms))
    return ms[0], ms[1], ms[2]


def corr_bwd(desc, code, code_pos, coords1, coords2, perms, saved, intra_cd, inter_cd, neg_cd,
             g_intra, g_inter, g_neg_loss, g_intra_cd, g_inter_cd, g_neg_cd, neg_is_mean=False):
    """stego_corr_bwd. g_* may be None. Returns (d_code, d_code_pos) as [B,K,H,W] views of channels-last buffers.
    neg_is_mean: g_neg_loss is ONE device scalar, the upstream of loss_means[2] (stride -1 of the C ABI)."""
    saved_w, saved_mean, saved_ctx = saved
    _require_dev(code, code_pos, saved_w)
    lib = load()
    dev = code.device
    B, K, H, W = desc.B, desc.K, desc.H, desc.W
    perms = _dense(perms, torch.int64) if desc.n_neg else None
    stride = 1
    if neg_is_mean:
        stride = -1
        g_neg_loss = None if g_neg_loss is None else _dense(g_neg_loss, torch.float32)
    elif g_neg_loss is not None and g_neg_loss.numel() > 0:
        if all(s == 0 for s in g_neg_loss.stride()):
            stride = 0                      # expanded scalar: hand over the one element
        else:
            g_neg_loss = _dense(g_neg_loss, torch.float32)
    else:
        g_neg_loss = None
    g_intra = None if g_intra is None else _dense(g_intra, torch.float32)
    g_inter = None if g_inter is None else _dense(g_inter, torch.float32)
    g_intra_cd = None if g_intra_cd is None else _dense(g_intra_cd, torch.float32)
    g_inter_cd = None if g_inter_cd is None else _dense(g_inter_cd, torch.float32)
    g_neg_cd = None if (g_neg_cd is None or g_neg_cd.numel() == 0) else _dense(g_neg_cd, torch.float32)
    d_code = torch.empty(B, H, W, K, dtype=torch.float32, device=dev)
    d_code_pos = torch.empty(B, H, W, K, dtype=torch.float32, device=dev)
    ws = _empty_bytes(lib.stego_corr_bwd_workspace_bytes(byref(desc)), dev)
    with _on_device(dev):
        _check(lib.stego_corr_bwd(byref(desc), _ptr(perms),
                                  _ptr(saved_w), _ptr(saved_mean), _ptr(saved_ctx),
                                  _ptr(intra_cd), _ptr(inter_cd), _ptr(neg_cd),
                                  _ptr(g_intra), _ptr(g_inter), _ptr(g_neg_loss), stride,
                                  _ptr(g_intra_cd), _ptr(g_inter_cd), _ptr(g_neg_cd),
                                  _ptr(d_code), _ptr(d_code_pos), _ptr(ws), ws.numel(), _stream()))
    return d_code.permute(0, 3, 1, 2), d_code_pos.permute(0, 3, 1, 2)


def helper_fwd(desc, f1, f2, c1, c2, need_grad):
    _require_dev(f1, f2, c1, c2)
    lib = load()
    N, S1, S2 = desc.B, desc.H, desc.W
    dev = f1.device
    f32 = dict(dtype=torch.float32, device=dev)
    loss = torch.empty(N, S1, S2, S1, S2, **f32)
    cd = torch.empty(N, S1, S2, S1, S2, **f32)
    saved_w = torch.empty(N, (S1 * S2) ** 2, **f32) if need_grad else None
    saved_mean = torch.empty(1, **f32) if need_grad else None
    saved_ctx = _empty_bytes(lib.stego_corr_helper_saved_ctx_bytes(byref(desc)), dev) if need_grad else None
    ws = _empty_bytes(lib.stego_corr_helper_workspace_bytes(byref(desc)), dev)
    m1, m2, m3, m4 = _map(f1), _map(f2), _map(c1), _map(c2)
    with _on_device(dev):
        _check(lib.stego_corr_helper_fwd(byref(desc), byref(m1), byref(m2), byref(m3), byref(m4),
                                         _ptr(loss), _ptr(cd), _ptr(saved_w), _ptr(saved_mean), _ptr(saved_ctx),
                                         _ptr(ws), ws.numel(), _stream()))
    return loss, cd, ((saved_w, saved_mean, saved_ctx) if need_grad else None)


def helper_bwd(desc, c1, c2, saved, cd, g_loss, g_cd):
    saved_w, saved_mean, saved_ctx = saved
    _require_dev(c1, c2, saved_w)
    lib = load()
    N, K, S1, S2 = desc.B, desc.K, desc.H, desc.W
    dev = c1.device
    g_loss = None if g_loss is None else _dense(g_loss, torch.float32)
    g_cd = None if g_cd is None else _dense(g_cd, torch.float32)
    d1 = torch.empty(N, S1, S2, K, dtype=torch.float32, device=dev)
    d2 = torch.empty(N, S1, S2, K, dtype=torch.float32, device=dev)
    ws = _empty_bytes(lib.stego_corr_helper_bwd_workspace_bytes(byref(desc)), dev)
    with _on_device(dev):
        _check(lib.stego_corr_helper_bwd(byref(desc), _ptr(saved_w), _ptr(saved_mean),
                                         _ptr(saved_ctx), _ptr(cd), _ptr(g_loss), _ptr(g_cd), _ptr(d1), _ptr(d2),
                                         _ptr(ws), ws.numel(), _stream()))
    return d1.permute(0, 3, 1, 2), d2.permute(0, 3, 1, 2)


def knn_topk(x, k=30, normalize=False, q_begin=0, q_count=None, return_sims=False):
    """All-pairs cosine top-k (reference precompute_knns.py:86-96) of the rows of ``x`` [N, D] (fp32, HIP device).
    Returns int64 [q_count, k] (and the fp32 similarities)."""
    _require_dev(x)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("knn_topk expects a 2-D float32 tensor")
    if x.stride(1) != 1:
        x = x.contiguous()
    lib = load()
    N, D = x.shape
    q_count = N - q_begin if q_count is None else q_count
    nws = lib.stego_knn_workspace_bytes(N, D, k, q_count)
    if nws == 0:
        raise RuntimeError("stego_knn_topk: unsupported shape (need 1 <= k <= 32, k <= N < 2^31)")
    dev = x.device
    ws = _empty_bytes(nws, dev)
    idx = torch.empty(q_count, k, dtype=torch.int64, device=dev)
    sims = torch.empty(q_count, k, dtype=torch.float32, device=dev) if return_sims else None
    with _on_device(dev):
        _check(lib.stego_knn_topk(_ptr(x), N, D, x.stride(0), k, 1 if normalize else 0, q_begin, q_count, _ptr(idx), _ptr(sims),
                                  _ptr(ws), ws.numel(), _stream()))
    return (idx, sims) if return_sims else idx


def dense_corr(a, b, normalize=False):
    """tensor_correlation (reference modules.py:283-284), optionally on norm()'ed maps: a [B,C,H1,W1], b [B,C,H2,W2]
    (fp32, HIP device, any strides) -> [B,H1,W1,H2,W2].  Forward only."""
    _require_dev(a, b)
    if a.dim() != 4 or b.dim() != 4 or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError("dense_corr expects two 4-D float32 maps")
    if a.shape[:2] != b.shape[:2]:
        raise ValueError("dense_corr: batch / channel mismatch %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    lib = load()
    B, C, H1, W1 = a.shape
    H2, W2 = b.shape[2:]
    dev = a.device
    out = torch.empty(B, H1, W1, H2, W2, dtype=torch.float32, device=dev)
    ws = _empty_bytes(lib.stego_dense_corr_workspace_bytes(B, C, H1, W1, H2, W2), dev)
    ma, mb = _map(a), _map(b)
    with _on_device(dev):
        _check(lib.stego_dense_corr(byref(ma), byref(mb), B, C, H1, W1, H2, W2, 1 if normalize else 0, _ptr(out), _ptr(ws),
                                    ws.numel(), _stream()))
    return out


DENSE_KERNELS = ("stream", "rowblock", "tile")      # STEGO_DENSE_* of include/stego_corr.h


def dense_corr_kernel(a, b):
    """The kernel dense_corr(a, b) would launch - "stream", "rowblock" or "tile" (stego_dense_corr_kernel: strides and shapes only,
    nothing is launched and no map data is read, so host tensors are taken as well)."""
    if a.dim() != 4 or b.dim() != 4 or a.shape[:2] != b.shape[:2]:
        raise ValueError("dense_corr_kernel expects two 4-D maps of one batch size and width")
    B, C, H1, W1 = a.shape
    H2, W2 = b.shape[2:]
    ma, mb = _map(a), _map(b)
    rc = load().stego_dense_corr_kernel(byref(ma), byref(mb), B, C, H1, W1, H2, W2)
    if rc < 0:
        _check(-rc)
    return DENSE_KERNELS[rc]


def sample(t, coords, index=None):
    """sample(t[index], coords) of the reference (modules.py:287-288) without the indexed copy of `t`: t [M, C, H, W] (fp32, HIP device, any
    strides), coords [Nc, S, S, 2], index int64 [N] or None (N = M) -> [N, C, S, S] (a view of channels-last rows [N, S*S, C]).  Row n
    uses the coordinates of row n % Nc."""
    _require_dev(t, coords)
    if t.dim() != 4 or t.dtype != torch.float32 or coords.dim() != 4 or coords.shape[-1] != 2 or coords.shape[1] != coords.shape[2]:
        raise ValueError("sample expects a float32 [M, C, H, W] map and [Nc, S, S, 2] coordinates")
    lib = load()
    M, C, H, W = t.shape
    S = int(coords.shape[1])
    N = M if index is None else int(index.numel())
    coords = coords.contiguous().float()
    if index is not None:
        index = index.contiguous().to(torch.int64)
    out = torch.empty(N, S * S, C, dtype=torch.float32, device=t.device)
    m = _map(t)
    with _on_device(t.device):
        _check(lib.stego_sample(byref(m), _ptr(index) if index is not None else None, N, C, H, W, _ptr(coords), int(coords.shape[0]), S,
                                _ptr(out), _stream()))
    return out.view(N, S, S, C).permute(0, 3, 1, 2)


def loss_pointwise_fwd(fd, cd, shifts, cmin, cmax, pointwise, rowsum=None):
    """The elementwise part of helper() (modules.py:330-345) over all pair-sets: fd, cd [n_sets, B, P, P] contiguous fp32 ->
    (neg_loss [n_sets - 2, B, P, P], per-set loss sums [n_sets], rowsum [n_sets * B * P], old_mean [n_sets]).  rowsum: the row sums of fd when
    the correlation kernel already took them (dense_corr_panels(want_rowsum=True))."""
    _require_dev(fd, cd)
    lib = load()
    n_sets, B, P = int(fd.shape[0]), int(fd.shape[1]), int(fd.shape[2])
    dev = fd.device
    rows = n_sets * B * P
    have_rowsum = rowsum is not None
    if not have_rowsum:
        rowsum = torch.empty(rows, dtype=torch.float32, device=dev)
    sh = (c_float * 3)(*[float(x) for x in shifts])
    neg_loss = torch.empty(max(n_sets - 2, 0), B, P, P, dtype=torch.float32, device=dev)
    loss_rowsum = torch.empty(rows, dtype=torch.float32, device=dev)
    with _on_device(dev):
        if pointwise:
            if not have_rowsum:
                _check(lib.stego_rowsum(_ptr(fd), rows, P, _ptr(rowsum), _stream()))
            old_mean = rowsum.view(n_sets, -1).sum(1) / float(B * P * P)
        else:
            old_mean = torch.zeros(n_sets, dtype=torch.float32, device=dev)
        _check(lib.stego_loss_pointwise_fwd(_ptr(fd), _ptr(cd), _ptr(rowsum), _ptr(old_mean), n_sets, B, P, sh, float(cmin), float(cmax),
                                            1 if pointwise else 0, _ptr(neg_loss) if n_sets > 2 else None, _ptr(loss_rowsum), _stream()))
    return neg_loss, loss_rowsum.view(n_sets, -1).sum(1), rowsum, old_mean


def loss_pointwise_bwd(fd, cd, rowsum, old_mean, shifts, cmin, cmax, pointwise, g_neg, g_sums):
    """d cd of loss_pointwise_fwd: g_neg (upstream of neg_loss: dense, an expanded scalar, or None), g_sums (upstream of the sums, or None)."""
    lib = load()
    n_sets, B, P = int(fd.shape[0]), int(fd.shape[1]), int(fd.shape[2])
    sh = (c_float * 3)(*[float(x) for x in shifts])
    g_cd = torch.empty_like(cd)
    dense = bcast = None
    if g_neg is not None and g_neg.numel() > 0:
        if all(st == 0 for st in g_neg.stride()):
            bcast = g_neg                                   # ONE value behind every element (the backward of .mean() / .sum())
        else:
            dense = g_neg.contiguous().float()
    if g_sums is not None:
        g_sums = g_sums.contiguous().float()
    with _on_device(fd.device):
        _check(lib.stego_loss_pointwise_bwd(_ptr(fd), _ptr(cd), _ptr(rowsum), _ptr(old_mean), n_sets, B, P, sh, float(cmin), float(cmax),
                                            1 if pointwise else 0, _ptr(dense) if dense is not None else None,
                                            _ptr(bcast) if bcast is not None else None, _ptr(g_sums) if g_sums is not None else None,
                                            _ptr(g_cd), _stream()))
    return g_cd


def sample_bwd(g_out, like, coords, index=None):
    """Adjoint of sample(): g_out [N, C, S, S] -> the gradient of the map (shape and memory format of `like`), atomic fp32 adds."""
    _require_dev(g_out, coords)
    lib = load()
    M, C, H, W = like.shape
    S = int(coords.shape[1])
    N = M if index is None else int(index.numel())
    g = g_out.permute(0, 2, 3, 1).contiguous()                     # [N, S, S, C] rows
    coords = coords.contiguous().float()
    if index is not None:
        index = index.contiguous().to(torch.int64)
    d = torch.zeros_like(like, dtype=torch.float32)               # (preserves the strides of a dense `like`: channels-last stays channels-last)
    m = _map(d)
    with _on_device(like.device):
        _check(lib.stego_sample_bwd(_ptr(g), byref(m), _ptr(index) if index is not None else None, N, C, H, W, _ptr(coords),
                                    int(coords.shape[0]), S, _stream()))
    return d


def sample_bwd_rows(g_rows, d_map, coords, index=None, rows_n=None, inv=None):
    """Adjoint of sample() for gradients that are already channels-last rows: g_rows [N, P, C] contiguous is ADDED into d_map (the map's
    gradient, fp32, any strides, zeroed by the caller).  With rows_n / inv (the normalised rows and 1 / max(|row|, eps) stego_sample_panels
    saved) g_rows is the gradient of the NORMALISED rows and the backward of norm() (F.normalize, modules.py:275-276) is applied on the way:
    d row = inv * (g - rows_n <rows_n, g>), or inv * g where the row's norm was below eps."""
    _require_dev(g_rows, d_map)
    lib = load()
    M, C, H, W = d_map.shape
    S = int(coords.shape[1])
    N = int(g_rows.shape[0])
    if g_rows.dim() != 3 or not g_rows.is_contiguous() or g_rows.shape[1] != S * S or g_rows.shape[2] != C or g_rows.dtype != torch.float32:
        raise ValueError("sample_bwd_rows expects contiguous float32 [N, S*S, C] rows")
    if (rows_n is None) != (inv is None) or (rows_n is not None and (not rows_n.is_contiguous() or not inv.is_contiguous()
                                                                   or rows_n.shape != g_rows.shape or inv.numel() != N * S * S)):
        raise ValueError("sample_bwd_rows: rows_n [N, P, C] and inv [N, P] go together, contiguous")
    coords = coords.contiguous().float()
    if index is not None:
        index = index.contiguous().to(torch.int64)
        if index.numel() != N:
            raise ValueError("sample_bwd_rows: one index per row image")
    elif N != M:
        raise ValueError("sample_bwd_rows: %d row images for a map of %d" % (N, M))
    m = _map(d_map)
    with _on_device(d_map.device):
        _check(lib.stego_sample_bwd_rows(_ptr(g_rows), _ptr(rows_n) if rows_n is not None else None, _ptr(inv) if inv is not None else None,
                                         byref(m), _ptr(index) if index is not None else None, N, C, H, W, _ptr(coords),
                                         int(coords.shape[0]), S, _stream()))
    return d_map


class PanelSet:
    """Prepared operands of the dense-correspondence kernel for `images` point sets of P points x C channels (include/stego_corr.h,
    stego_sample_panels): split-fp16 operand images + one scale per row."""

    def __init__(self, images, C, P, device):
        lib = load()
        self.images, self.C, self.P = int(images), int(C), int(P)
        self.image_bytes = int(lib.stego_panel_image_bytes(self.C, self.P))
        if self.image_bytes <= 0:
            raise ValueError("PanelSet: bad shape C = %d, P = %d" % (C, P))
        self.rows = (self.P + 127) // 128 * 128
        self.panels = torch.empty(self.images * self.image_bytes, dtype=torch.uint8, device=device)
        self.row_scale = torch.empty(self.images, self.rows, dtype=torch.float32, device=device)


def sample_panels(pset, first, t, coords, index=None, normalize=True, rows_out=None, inv_out=None):
    """Images [first, first + N) of `pset` = norm(sample(t if index is None else t[index], coords)) (modules.py:275-276, 287-288, 384-385) as
    operands of dense_corr_panels; rows_out [N, P, C] / inv_out [N, P] (contiguous fp32, optional) receive the normalised rows and
    1 / max(|row|, eps)."""
    _require_dev(t, coords)
    if t.dim() != 4 or t.dtype != torch.float32 or coords.dim() != 4 or coords.shape[-1] != 2 or coords.shape[1] != coords.shape[2]:
        raise ValueError("sample_panels expects a float32 [M, C, H, W] map and [Nc, S, S, 2] coordinates")
    lib = load()
    M, C, H, W = t.shape
    S = int(coords.shape[1])
    N = M if index is None else int(index.numel())
    if C != pset.C or S * S != pset.P or first < 0 or first + N > pset.images:
        raise ValueError("sample_panels: the panel set holds %d images of %d x %d" % (pset.images, pset.P, pset.C))
    for o, shape in ((rows_out, (N, S * S, C)), (inv_out, (N, S * S))):
        if o is not None and (tuple(o.shape) != shape or not o.is_contiguous() or o.dtype != torch.float32):
            raise ValueError("sample_panels: optional outputs are contiguous float32 %s" % (shape,))
    coords = coords.contiguous().float()
    if index is not None:
        index = index.contiguous().to(torch.int64)
    m = _map(t)
    with _on_device(t.device):
        _check(lib.stego_sample_panels(byref(m), _ptr(index) if index is not None else None, N, C, H, W, _ptr(coords), int(coords.shape[0]), S,
                                       1 if normalize else 0, pset.panels.data_ptr() + first * pset.image_bytes, _ptr(pset.row_scale[first:]),
                                       _ptr(rows_out) if rows_out is not None else None, _ptr(inv_out) if inv_out is not None else None, _stream()))


def dense_corr_panels(pa, images_a, pb, N, want_rowsum=False):
    """out[n] = (image n % images_a of pa) . (image n of pb)^T, [N, P, P] fp32: tensor_correlation (modules.py:283-284) of one set of anchors
    against the second operands of N / images_a pair-sets.  want_rowsum: also returns sum_j out[n, i, j] as [N * P]."""
    lib = load()
    if pa.C != pb.C or images_a > pa.images or N > pb.images or images_a < 1 or N < 1:
        raise ValueError("dense_corr_panels: operand sets do not match")
    out = torch.empty(N, pa.P, pb.P, dtype=torch.float32, device=pa.panels.device)
    rowsum = torch.empty(N * pa.P, dtype=torch.float32, device=out.device) if want_rowsum else None
    with _on_device(out.device):
        _check(lib.stego_dense_corr_panels(_ptr(pa.panels), _ptr(pa.row_scale), images_a, _ptr(pb.panels), _ptr(pb.row_scale), N, pa.C, pa.P, pb.P,
                                           _ptr(out), _ptr(rowsum), _stream()))
    return (out, rowsum) if want_rowsum else out


# ------------------------------------------------------------------ segmentation head (include/stego_head.h)
def head_desc(tokens, K, nonlinear):
    """tokens: fp32 [B, HW, C] view with a dense channel axis (e.g. feat[:, 1:, :] of the backbone: the class token is skipped by
    the view's offset, the image stride stays (1 + HW) * C)."""
    if tokens.dim() != 3 or tokens.dtype != torch.float32 or tokens.stride(2) != 1:
        raise RuntimeError("head: expected a float32 [B, HW, C] token tensor with contiguous channels")
    B, HW, C = tokens.shape
    return StegoHeadDesc(B, HW, C, int(K), 1 if nonlinear else 0, tokens.stride(1), tokens.stride(0) if B > 1 else HW * tokens.stride(1), None)


def tokens_from_cache(table, index, skip_rows=1):
    """stego_tokens_from_cache: float32 [n, ntok, D] rows `index` of the fp16 token table + a device word (int32 [1]) with the float bits
    of the largest magnitude of the rows >= skip_rows (what StegoHeadDesc.tokens_amax takes)."""
    _require_dev(table, index)
    if table.dtype != torch.float16 or table.dim() != 3 or not table.is_contiguous():
        raise RuntimeError("tokens_from_cache: expected a contiguous float16 [items, ntok, D] table")
    lib = load()
    dev = table.device
    index = _dense(index, torch.int64)
    n, ntok, D = int(index.numel()), table.shape[1], table.shape[2]
    out = torch.empty(n, ntok, D, dtype=torch.float32, device=dev)
    amax = torch.empty(1, dtype=torch.int32, device=dev)
    with _on_device(dev):
        _check(lib.stego_tokens_from_cache(_ptr(table), _ptr(index), n, ntok, D, int(skip_rows), _ptr(out), _ptr(amax), _stream()))
    return out, amax


def head_fwd(tokens, masks, w1, b1, w21, b21, w22, b22, need_grad, want_feats, tokens_amax=None):
    """stego_head_fwd.  masks = (m1, m2, m3) fp32 [B, C] each or None.  Returns (code [B, HW, K], feats_out [B, HW, C] or None,
    saved_h or None)."""
    _require_dev(tokens, w1, b1)
    lib = load()
    dev = tokens.device
    nonlinear = w21 is not None
    d = head_desc(tokens, w1.shape[0], nonlinear)
    if tokens_amax is not None:                  # (the magnitude word of exactly these tokens: tokens_from_cache)
        d.tokens_amax = tokens_amax.data_ptr()
    B, HW, C, K = d.B, d.HW, d.C, d.K
    code = torch.empty(B, HW, K, dtype=torch.float32, device=dev)
    feats = torch.empty(B, HW, C, dtype=torch.float32, device=dev) if want_feats else None
    saved_h = torch.empty(B * HW * C + 8, dtype=torch.float32, device=dev) if (nonlinear and need_grad) else None
    nws = int(lib.stego_head_fwd_workspace_bytes(byref(d)))
    if nws == 0:
        raise RuntimeError("stego_head_fwd: unsupported shape (C a multiple of 32, K <= 128, 16-byte token rows)")
    if nonlinear and saved_h is not None:       # H lives in saved_h: the workspace only holds the scale words and the split weights
        nws -= (B * HW * C * 4 + 255) // 256 * 256
    ws = _empty_bytes(nws, dev)
    m1, m2, m3 = masks if masks is not None else (None, None, None)
    with _on_device(dev):
        _check(lib.stego_head_fwd(byref(d), _ptr(tokens), _ptr(m1), _ptr(m2), _ptr(m3), _ptr(w1), _ptr(b1), _ptr(w21), _ptr(b21),
                                  _ptr(w22), _ptr(b22), _ptr(code), _ptr(feats), _ptr(saved_h), _ptr(ws), ws.numel(), _stream()))
    return code, feats, saved_h


def head_bwd(tokens, masks, saved_h, w22, d_code, K):
    """stego_head_bwd -> (dw1, db1, dw21, db21, dw22, db22) (the cluster2 entries None for a linear head)."""
    _require_dev(tokens, d_code)
    lib = load()
    dev = tokens.device
    nonlinear = saved_h is not None
    d = head_desc(tokens, K, nonlinear)
    C = d.C
    f32 = dict(dtype=torch.float32, device=dev)
    dw1, db1 = torch.empty(K, C, **f32), torch.empty(K, **f32)
    dw21 = db21 = dw22 = db22 = None
    if nonlinear:
        dw21, db21, dw22, db22 = torch.empty(C, C, **f32), torch.empty(C, **f32), torch.empty(K, C, **f32), torch.empty(K, **f32)
    d_code = _dense(d_code, torch.float32)
    ws = _empty_bytes(lib.stego_head_bwd_workspace_bytes(byref(d)), dev)
    m1, m2 = (masks[0], masks[1]) if masks is not None else (None, None)
    with _on_device(dev):
        _check(lib.stego_head_bwd(byref(d), _ptr(tokens), _ptr(m1), _ptr(m2), _ptr(saved_h), _ptr(w22), _ptr(d_code),
                                  _ptr(dw1), _ptr(db1), _ptr(dw21), _ptr(db21), _ptr(dw22), _ptr(db22), _ptr(ws), ws.numel(), _stream()))
    return dw1, db1, dw21, db21, dw22, db22


# (every NAME_workspace_bytes below: host only, 0 for an invalid descriptor)
crf_desc = _desc(StegoCrfDesc)
crf_workspace_bytes = _bytes("stego_crf_workspace_bytes")


def crf_run(desc, bgr_u8, probs, keep_workspace=False, workspace=None):
    """stego_crf_run: bgr_u8 [B,H,W,3] uint8 and probs [B,C,H,W] float32, contiguous on one HIP device -> Q [B,C,H,W] float32
    (and the workspace, for crf_lattice_info, with keep_workspace).  `workspace`: a uint8 device tensor of at least
    crf_workspace_bytes(desc) bytes to use instead of a fresh one."""
    _require_dev(bgr_u8, probs)
    lib = load()
    dev = probs.device
    q = torch.empty(tuple(probs.shape), dtype=torch.float32, device=dev)
    ws = workspace if workspace is not None else _empty_bytes(max(int(lib.stego_crf_workspace_bytes(byref(desc))), 256), dev)
    nbytes = ws.numel()
    with _on_device(dev):
        _check(lib.stego_crf_run(byref(desc), _ptr(bgr_u8), _ptr(probs), _ptr(q), _ptr(ws), nbytes, _stream()))
    return (q, ws) if keep_workspace else q


def crf_lattice_info(desc, ws, b, which, max_keys=0):
    """(vertex count, the first max_keys packed vertex keys as uint64 numpy) of lattice `which` (0 Gaussian, 1 bilateral) of image b."""
    import numpy as np
    lib = load()
    n = c_int32(0)
    keys = np.zeros(max(int(max_keys), 1), dtype=np.uint64)
    with _on_device(ws.device):
        _check(lib.stego_crf_lattice_info(byref(desc), _ptr(ws), ws.numel(), int(b), int(which), byref(n),
                                          keys.ctypes.data if max_keys else None, int(max_keys), _stream()))
    return n.value, keys[:min(n.value, int(max_keys))]


# ---- batch preparation of the device image store (include/stego_data.h; stego_amd.device_data builds the table and the arenas)
data_desc = _desc(StegoDataDesc)


def data_check_items(desc, items_np):
    """stego_data_check_items on a host numpy array of StegoDataItem records (host only) -> (rc, first bad record or -1)."""
    bad = c_int64(-1)
    rc = load().stego_data_check_items(byref(desc), items_np.ctypes.data, byref(bad))
    return int(rc), int(bad.value)


def data_prepare_raw(desc, items, img_arena, label_arena, map_pool, lut, index, origin, img, label, mask):
    """stego_data_prepare with every buffer given (tests: the error codes) -> the return code, unchecked."""
    with _on_device(img.device if img is not None else index.device):
        return int(load().stego_data_prepare(byref(desc), _ptr(items), _ptr(img_arena), _ptr(label_arena), _ptr(map_pool), _ptr(lut),
                                             _ptr(index), _ptr(origin), _ptr(img), _ptr(label), _ptr(mask), _stream()))


def data_prepare(desc_args, items, img_arena, label_arena, map_pool, lut, index, origin=None):
    """stego_data_prepare: index int64 [N] and origin int32 [N, 2] (or None: centre crops) on the device of the arenas ->
    (img float32 [N,3,R,R], label int64 [N,R,R], mask bool [N,1,R,R]).  desc_args = (R, n_items, img bytes, label bytes, pool len)."""
    _require_dev(items, img_arena, label_arena, map_pool, lut, index, origin)
    R = int(desc_args[0])
    N = int(index.numel())
    dev = index.device
    desc = data_desc(N, *desc_args)
    img = torch.empty(N, 3, R, R, dtype=torch.float32, device=dev)
    label = torch.empty(N, R, R, dtype=torch.int64, device=dev)
    mask = torch.empty(N, 1, R, R, dtype=torch.bool, device=dev)
    _check(data_prepare_raw(desc, items, img_arena, label_arena, map_pool, lut, index, origin, img, label, mask))
    return img, label, mask


def data_prepare_dir_raw(desc, items, img_arena, label_arena, map_pool, lut, index, origin, img, label, mask):
    """stego_data_prepare_dir with every buffer given (label_arena None: a store without labels) -> the return code, unchecked."""
    with _on_device(img.device if img is not None else index.device):
        return int(load().stego_data_prepare_dir(byref(desc), _ptr(items), _ptr(img_arena), _ptr(label_arena), _ptr(map_pool), _ptr(lut),
                                                 _ptr(index), _ptr(origin), _ptr(img), _ptr(label), _ptr(mask), _stream()))


def data_prepare_dir(desc_args, items, img_arena, label_arena, map_pool, lut, index, origin=None):
    """stego_data_prepare_dir (a directory store; label_arena None when the folder has no labels): as data_prepare, with
    label = the stored byte (or -1) and mask float32 [N,1,R,R] = label > 0."""
    _require_dev(items, img_arena, label_arena, map_pool, lut, index, origin)
    R = int(desc_args[0])
    N = int(index.numel())
    dev = index.device
    desc = data_desc(N, *desc_args)
    img = torch.empty(N, 3, R, R, dtype=torch.float32, device=dev)
    label = torch.empty(N, R, R, dtype=torch.int64, device=dev)
    mask = torch.empty(N, 1, R, R, dtype=torch.float32, device=dev)
    _check(data_prepare_dir_raw(desc, items, img_arena, label_arena, map_pool, lut, index, origin, img, label, mask))
    return img, label, mask


# ---- salience-guided coordinate draws (include/stego_salience.h; modules.ContrastiveCorrelationLoss.draw with cfg.native_salience)
def salience_covers(B, H, W, S):
    """The limits of stego_salience_coords (anything else keeps the torch path)."""
    return 1 <= S <= SALIENCE_MAX_S and 1 <= B <= SALIENCE_MAX_B and H >= 1 and W >= 1 and H * W <= SALIENCE_MAX_PIXELS


def salience_coords(mask1, mask2, u, u_mix, reg1, reg2):
    """stego_salience_coords: mask1 / mask2 [B, H, W] (uint8, bool or float32), u float32 [2, B, S, S, 3], u_mix float32 [B, S, S],
    reg1 / reg2 float32 [B, S, S, 2] -> (coords1, coords2) float32 [B, S, S, 2].  One launch, no host synchronisation."""
    _require_dev(mask1, mask2, u, u_mix, reg1, reg2)
    B, H, W = mask1.shape
    S = int(u_mix.shape[1])
    if mask1.dtype != mask2.dtype or mask1.shape != mask2.shape:
        raise ValueError("the two salience masks differ in dtype or shape: %s %s, %s %s"
                         % (mask1.dtype, tuple(mask1.shape), mask2.dtype, tuple(mask2.shape)))
    if mask1.dtype == torch.float32:
        kind = SALIENCE_F32
    elif mask1.dtype in (torch.uint8, torch.bool):
        kind = SALIENCE_U8
    else:
        raise ValueError("salience masks must be uint8, bool or float32, got %s" % mask1.dtype)
    if tuple(u.shape) != (2, B, S, S, 3) or tuple(u_mix.shape) != (B, S, S) or tuple(reg1.shape) != (B, S, S, 2) or \
            tuple(reg2.shape) != (B, S, S, 2) or any(t.dtype != torch.float32 for t in (u, u_mix, reg1, reg2)):
        raise ValueError("salience_coords: u [2,B,S,S,3], u_mix [B,S,S], reg [B,S,S,2] float32 expected for B = %d, S = %d" % (B, S))
    mask1, mask2, u, u_mix, reg1, reg2 = (t.contiguous() for t in (mask1, mask2, u, u_mix, reg1, reg2))
    coords1, coords2 = torch.empty_like(reg1), torch.empty_like(reg2)
    desc = StegoSalienceDesc(int(B), int(H), int(W), S, kind)
    with _on_device(mask1.device):
        _check(load().stego_salience_coords(byref(desc), _ptr(mask1), _ptr(mask2), _ptr(u), _ptr(u_mix), _ptr(reg1), _ptr(reg2),
                                            _ptr(coords1), _ptr(coords2), _stream()))
    return coords1, coords2


# ---- fused probe head (include/stego_probe.h; stego_amd.segment wraps it for a model)
probe_desc = _desc(StegoProbeDesc)
probe_head_raw = _raw("stego_probe_head")


def probe_head_plan(desc):
    """stego_probe_head_plan (host only) -> (LDS bytes, tile rows, tile columns); 0 bytes for an invalid descriptor."""
    ty, tx = c_int32(0), c_int32(0)
    n = load().stego_probe_head_plan(byref(desc), byref(ty), byref(tx))
    return int(n), ty.value, tx.value


def _probe_weights(lin_w, lin_b, centroids, n_lin, n_clu, K):
    """The probes' weights as dense float32 tensors, None for a skipped probe (n == 0); their shapes checked against K."""
    def weights(t, n):
        return _dense(t, torch.float32) if t is not None and n else None
    lw, lb, ce = weights(lin_w, n_lin), weights(lin_b, n_lin), weights(centroids, n_clu)
    if lw is not None and tuple(lw.shape) != (n_lin, K) or ce is not None and tuple(ce.shape) != (n_clu, K):
        raise ValueError("probe weights %s / %s do not match K = %d" % (None if lw is None else tuple(lw.shape),
                                                                        None if ce is None else tuple(ce.shape), K))
    return lw, lb, ce


def _probe_out(kind, n, lead, H, W, dev):
    """A probe's output: None when skipped, int64 [*lead, H, W] for "argmax", else float32 [*lead, n, H, W]."""
    if kind == PROBE_SKIP:
        return None
    if kind == PROBE_ARGMAX:
        return torch.empty(*lead, H, W, dtype=torch.int64, device=dev)
    return torch.empty(*lead, n, H, W, dtype=torch.float32, device=dev)


def probe_head(code, code_flip, lin_w, lin_b, centroids, size, lin_kind, clu_kind, alpha):
    """stego_probe_head: code (and code_flip, or None) float32 [B, K, h, w] with any strides, lin_w [n_lin, K], lin_b [n_lin],
    centroids [n_clu, K] (L2-normalised) on one HIP device -> (linear output, cluster output), each None for a skipped probe,
    float32 [B, n, H, W] for "log_probs" / "probs" and int64 [B, H, W] for "argmax"."""
    _require_dev(code, code_flip, lin_w, lin_b, centroids)
    B, K, h, w = code.shape
    H, W = int(size[0]), int(size[1])
    lk, ck = PROBE_KINDS[lin_kind], PROBE_KINDS[clu_kind]
    n_lin = int(lin_w.shape[0]) if lk != PROBE_SKIP else 0
    n_clu = int(centroids.shape[0]) if ck != PROBE_SKIP else 0
    if code_flip is not None and tuple(code_flip.shape) != tuple(code.shape):
        raise ValueError("code_flip %s does not match code %s" % (tuple(code_flip.shape), tuple(code.shape)))
    dev = code.device
    lw, lb, ce = _probe_weights(lin_w, lin_b, centroids, n_lin, n_clu, K)
    lo, co = _probe_out(lk, n_lin, (B,), H, W, dev), _probe_out(ck, n_clu, (B,), H, W, dev)
    desc = probe_desc(B, K, h, w, H, W, n_lin, n_clu, lk, ck, alpha)
    with _on_device(dev):
        _check(probe_head_raw(desc, _map(code), _map(code_flip) if code_flip is not None else None, lw, lb, ce, lo, co, _stream()))
    return lo, co


# ---- sliding windows stitched on the canvas (include/stego_stitch.h; stego_amd.segment.segment_large wraps them for a model)
window_layout = _desc(StegoWindowLayout)
stitch_probe_raw = _raw("stego_stitch_probe")
window_gather_raw = _raw("stego_window_gather")


def stitch_desc(H, W, win, stride, T, K, hc, wc, n_lin, n_clu, lin_kind, clu_kind, alpha):
    return StegoStitchDesc(window_layout(H, W, win, stride), int(T), int(K), int(hc), int(wc), int(n_lin), int(n_clu), int(lin_kind),
                           int(clu_kind), float(alpha))


def stitch_probe_plan(desc):
    """stego_stitch_probe_plan (host only) -> (LDS bytes, tile rows, tile columns, ny, nx); 0 bytes for an invalid descriptor."""
    ty, tx, ny, nx = c_int32(0), c_int32(0), c_int32(0), c_int32(0)
    n = load().stego_stitch_probe_plan(byref(desc), byref(ty), byref(tx), byref(ny), byref(nx))
    return int(n), ty.value, tx.value, ny.value, nx.value


def stitch_probe(code, code_flip, lin_w, lin_b, centroids, size, win, stride, lin_kind, clu_kind, alpha):
    """stego_stitch_probe: the codes of the canvas's windows (and of their mirror images, or None) float32 [T, K, hc, wc] with any
    strides, window t = iy * nx + ix at index t; the probes' weights as for probe_head; `size` = (H, W) of the canvas, `win` and
    `stride` its window layout -> (linear output, cluster output) on the canvas, each None for a skipped probe, float32 [n, H, W] for
    "log_probs" / "probs" and int64 [H, W] for "argmax"."""
    _require_dev(code, code_flip, lin_w, lin_b, centroids)
    T, K, hc, wc = code.shape
    H, W = int(size[0]), int(size[1])
    lk, ck = PROBE_KINDS[lin_kind], PROBE_KINDS[clu_kind]
    n_lin = int(lin_w.shape[0]) if lk != PROBE_SKIP else 0
    n_clu = int(centroids.shape[0]) if ck != PROBE_SKIP else 0
    if code_flip is not None and tuple(code_flip.shape) != tuple(code.shape):
        raise ValueError("code_flip %s does not match code %s" % (tuple(code_flip.shape), tuple(code.shape)))
    dev = code.device
    lw, lb, ce = _probe_weights(lin_w, lin_b, centroids, n_lin, n_clu, K)
    desc = stitch_desc(H, W, win, stride, T, K, hc, wc, n_lin, n_clu, lk, ck, alpha)
    if stitch_probe_plan(desc)[0] == 0:     # an invalid descriptor: name the error before any output is sized from it
        _check(stitch_probe_raw(desc, None, None, None, None, None, None, None))
    lo, co = _probe_out(lk, n_lin, (), H, W, dev), _probe_out(ck, n_clu, (), H, W, dev)
    with _on_device(dev):
        _check(stitch_probe_raw(desc, _map(code), _map(code_flip) if code_flip is not None else None, lw, lb, ce, lo, co, _stream()))
    return lo, co


def window_gather(img, win, stride, t0, n, flip=False):
    """stego_window_gather: windows [t0, t0 + n) of the float32 image [3, H, W] (any strides) -> float32 [n, 3, win, win], and with
    `flip` also their horizontal mirror images: (windows, mirrored windows)."""
    _require_dev(img)
    if img.dtype != torch.float32 or img.dim() != 3 or img.shape[0] != 3:
        raise ValueError("img: expected a float32 [3, H, W] tensor, got %s %s" % (img.dtype, tuple(img.shape)))
    H, W = int(img.shape[1]), int(img.shape[2])
    dev = img.device
    layout = window_layout(H, W, win, stride)
    shape = (max(int(n), 0), 3, max(int(win), 0), max(int(win), 0))
    ok = window_gather_raw(layout, None, t0, n, None, None) == 1       # only the pointers are missing
    out = torch.empty(shape if ok else (0,), dtype=torch.float32, device=dev)
    out_flip = torch.empty(shape if ok else (0,), dtype=torch.float32, device=dev) if flip else None
    with _on_device(dev):
        _check(window_gather_raw(layout, _map(img.unsqueeze(0)), t0, n, out, out_flip, _stream()))
    return (out, out_flip) if flip else out


# ---- coloured pictures (include/stego_render.h; stego_amd.render wraps them for label maps, images and contact sheets)
def render_desc(B, H, W, n_lut=1, label_dtype=RENDER_I64, flags=RENDER_LABELS, alpha=0.0, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0),
                ignore_rgb=(0, 0, 0), edge_rgb=(0, 0, 0), label_strides=(0, 0, 1), out_strides=(0, 0)):
    d = StegoRenderDesc(int(B), int(H), int(W), int(n_lut), int(label_dtype), int(flags), float(alpha))
    for c in range(3):
        d.mean[c], d.std[c] = float(mean[c]), float(std[c])
        d.ignore_rgb[c], d.edge_rgb[c] = int(ignore_rgb[c]), int(edge_rgb[c])
    d.label_stride_n, d.label_stride_h, d.label_stride_w = (int(v) for v in label_strides)
    d.out_stride_n, d.out_stride_h = (int(v) for v in out_strides)
    return d


image_range_workspace_bytes = _bytes("stego_image_range_workspace_bytes")
image_range_raw = _raw("stego_image_range")
render_raw = _raw("stego_render")


def image_range(desc, image):
    """stego_image_range of the float32 image [B, 3, H, W] (any strides) -> float32 [B, 2], (lo, hi) per image."""
    _require_dev(image)
    dev = image.device
    ws, need = _workspace(image_range_workspace_bytes, desc, dev, lambda: image_range_raw(desc, None, None, None, 0))
    rng = torch.empty((desc.B, 2), dtype=torch.float32, device=dev)
    with _on_device(dev):
        _check(image_range_raw(desc, _map(image), rng, ws, need, _stream()))
    return rng


def render(desc, image, labels, lut, rng, out):
    """stego_render on torch's current stream: `out` is a uint8 tensor whose first element is the target's base (the descriptor holds
    its strides)."""
    _require_dev(image, labels, lut, rng, out)
    with _on_device(out.device):
        _check(render_raw(desc, _map(image) if image is not None else None, labels, lut, rng, out, _stream()))


# ---- feature pictures (include/stego_pca.h; stego_amd.feature_pca wraps them)
def pca_desc(B, C, h, w, H=1, W=1, joint=False, n_iter=PCA_DEFAULT_ITER, resize=PCA_BILINEAR, scale=PCA_UNIT, out_strides=(0, 0)):
    return StegoPcaDesc(int(B), int(C), int(h), int(w), int(H), int(W), PCA_JOINT if joint is True else PCA_PER_IMAGE if joint is False
                        else int(joint), int(n_iter), int(resize), int(scale), int(out_strides[0]), int(out_strides[1]))


pca_workspace_bytes = _bytes("stego_pca_workspace_bytes")
pca_fit_raw = _raw("stego_pca_fit")
pca_scores_raw = _raw("stego_pca_scores")
pca_paint_raw = _raw("stego_pca_paint")


def _pca_workspace(desc, dev):
    return _workspace(pca_workspace_bytes, desc, dev, lambda: pca_paint_raw(desc, None, None, None))


def pca_fit(desc, fmap):
    """Stages (a) - (c) of include/stego_pca.h on torch's current stream -> (mean [G, C], cov float64 [G, C, C], basis [G, 3, C],
    stats [G, 3, 3]), nothing synchronised."""
    _require_dev(fmap)
    dev = fmap.device
    G, C = (1 if desc.group == PCA_JOINT else desc.B), desc.C
    ws, need = _pca_workspace(desc, dev)
    mean = torch.empty((G, C), dtype=torch.float32, device=dev)
    cov = torch.empty((G, C, C), dtype=torch.float64, device=dev)
    basis = torch.empty((G, 3, C), dtype=torch.float32, device=dev)
    stats = torch.empty((G, 3, 3), dtype=torch.float32, device=dev)
    with _on_device(dev):
        _check(pca_fit_raw(desc, _map(fmap), mean, cov, basis, stats, ws, need, _stream()))
    return mean, cov, basis, stats


def pca_scores(desc, fmap, mean, basis):
    """Stage (d) -> (scores [B, h, w, 3], range [G, 3, 2])."""
    _require_dev(fmap, mean, basis)
    dev = fmap.device
    G = 1 if desc.group == PCA_JOINT else desc.B
    ws, need = _pca_workspace(desc, dev)
    scores = torch.empty((desc.B, desc.h, desc.w, 3), dtype=torch.float32, device=dev)
    rng = torch.empty((G, 3, 2), dtype=torch.float32, device=dev)
    with _on_device(dev):
        _check(pca_scores_raw(desc, _map(fmap), mean, basis, scores, rng, ws, need, _stream()))
    return scores, rng


def pca_paint(desc, scores, rng, out):
    """Stage (e): `out` is a uint8 tensor whose first element is the target's base (the descriptor holds its strides)."""
    _require_dev(scores, rng, out)
    with _on_device(out.device):
        _check(pca_paint_raw(desc, scores, rng, out, _stream()))


# ---- cluster refit (include/stego_kmeans.h; stego_amd.cluster_refit wraps them)
kmeans_desc = _desc(StegoKmeansDesc)
kmeans_workspace_bytes = _bytes("stego_kmeans_workspace_bytes")
kmeans_step_raw = _raw("stego_kmeans_step")
kmeans_seed_raw = _raw("stego_kmeans_seed")      # (`u`: a host array of doubles)


def kmeans_plan(desc):
    """stego_kmeans_plan (host only) -> (LDS bytes of the main launch, its workgroups); zeros for an invalid descriptor."""
    wgs = c_int32(-1)
    lds = load().stego_kmeans_plan(byref(desc), byref(wgs))
    return int(lds), int(wgs.value)


def kmeans_workspace(desc, dev):
    """(workspace tensor, its bytes) for kmeans_step / kmeans_seed calls with this descriptor."""
    return _workspace(kmeans_workspace_bytes, desc, dev, lambda: kmeans_step_raw(desc, None, None, None, None, None, None, None, 0))


_kmeans_workspace = kmeans_workspace


def kmeans_step(desc, codes, cin, cout=None, labels=None, counts=None, stats=None, workspace=None):
    """One Lloyd iteration of include/stego_kmeans.h on torch's current stream, nothing synchronised.  cout: float32 [n, K] (may be
    `cin`) or None for assignment only; labels: uint8 [B, h, w] or None; counts int64 [n] and stats float64 [4] are made when None;
    workspace: what kmeans_workspace(desc, device) returned, for callers that step repeatedly.  -> (counts, stats)."""
    _require_dev(codes, cin, cout, labels, counts, stats)
    dev = codes.device
    ws, need = workspace if workspace is not None else kmeans_workspace(desc, dev)
    if counts is None:
        counts = torch.empty((desc.n,), dtype=torch.int64, device=dev)
    if stats is None:
        stats = torch.empty((4,), dtype=torch.float64, device=dev)
    for name, t_, shape, dtype in (("centroids", cin, (desc.n, desc.K), torch.float32), ("out", cout, (desc.n, desc.K), torch.float32),
                                   ("labels", labels, (desc.B, desc.h, desc.w), torch.uint8), ("counts", counts, (desc.n,), torch.int64),
                                   ("stats", stats, (4,), torch.float64)):
        if t_ is not None:
            _expect("kmeans_step", name, t_, dtype, shape)
    with _on_device(dev):
        _check(kmeans_step_raw(desc, _map(codes), cin, cout, labels, counts, stats, ws, need, _stream()))
    return counts, stats


def kmeans_seed(desc, codes, u, workspace=None):
    """k-means++ seeding of include/stego_kmeans.h: `u` is a sequence of n numbers in [0, 1) -> (centroids float32 [n, K], picks int64
    [n]) on the codes' device, nothing synchronised."""
    _require_dev(codes)
    dev = codes.device
    ws, need = workspace if workspace is not None else kmeans_workspace(desc, dev)
    draws = (ctypes.c_double * desc.n)(*[float(v) for v in u])
    cent = torch.empty((desc.n, desc.K), dtype=torch.float32, device=dev)
    picks = torch.empty((desc.n,), dtype=torch.int64, device=dev)
    with _on_device(dev):
        _check(kmeans_seed_raw(desc, _map(codes), draws, cent, picks, ws, need, _stream()))
    return cent, picks


# ---- segments as objects (include/stego_regions.h; stego_amd.regions wraps them)
regions_desc = _desc(StegoRegionsDesc, connectivity=4, label_dtype=REGIONS_I64)
regions_workspace_bytes = _bytes("stego_regions_workspace_bytes")
regions_label_raw = _raw("stego_regions_label")
regions_table_raw = _raw("stego_regions_table")
regions_votes_raw = _raw("stego_regions_votes")
regions_relabel_raw = _raw("stego_regions_relabel")


def regions_plan(desc):
    """stego_regions_plan (host only) -> (return code, tile edge, [(LDS bytes, workgroups) of the six launches of regions_label])."""
    tile = c_int32(-1)
    lds, wgs = (c_size_t * REGIONS_LAUNCHES)(), (c_int64 * REGIONS_LAUNCHES)()
    rc = load().stego_regions_plan(byref(desc), byref(tile), lds, wgs)
    return int(rc), int(tile.value), [(int(a), int(b)) for a, b in zip(lds, wgs)]


def _regions_desc_of(labels, connectivity):
    if labels.dim() != 3 or labels.dtype not in REGIONS_DTYPES or not labels.is_contiguous():
        raise RuntimeError("regions: labels must be a contiguous int64, int32 or uint8 [B, H, W] tensor, got %s %s"
                           % (labels.dtype, tuple(labels.shape)))
    B, H, W = labels.shape
    return regions_desc(B, H, W, connectivity, REGIONS_DTYPES[labels.dtype])


def regions_label(labels, connectivity=4):
    """stego_regions_label on torch's current stream, nothing synchronised -> (ids int32 [B, H, W], n_regions int32 [B], root int32
    [B, H, W])."""
    _require_dev(labels)
    desc = _regions_desc_of(labels, connectivity)
    dev = labels.device
    ws, need = _workspace(regions_workspace_bytes, desc, dev, lambda: _call("stego_regions_plan", desc, None, None, None))
    ids = torch.empty(labels.shape, dtype=torch.int32, device=dev)
    root = torch.empty(labels.shape, dtype=torch.int32, device=dev)
    n_regions = torch.empty((labels.shape[0],), dtype=torch.int32, device=dev)
    with _on_device(dev):
        _check(regions_label_raw(desc, labels, ids, n_regions, root, ws, need, _stream()))
    return ids, n_regions, root


def regions_table(labels, ids, row_offset, capacity):
    """stego_regions_table -> (cols32 int32 [6, capacity]: area, y0, x0, y1, x1, first; cols64 int64 [3, capacity]: label, sum_y, sum_x).
    row_offset: int64 [B], the first row of every image."""
    _require_dev(labels, ids, row_offset)
    desc = _regions_desc_of(labels, 4)
    _expect("regions", "ids", ids, torch.int32, labels.shape)
    _expect("regions", "row_offset", row_offset, torch.int64, (labels.shape[0],))
    dev = labels.device
    cols32 = torch.empty((len(REGIONS_COLS32), int(capacity)), dtype=torch.int32, device=dev)
    cols64 = torch.empty((len(REGIONS_COLS64), int(capacity)), dtype=torch.int64, device=dev)
    with _on_device(dev):
        _check(regions_table_raw(desc, labels, ids, row_offset, capacity, cols32, cols64, _stream()))
    return cols32, cols64


def regions_votes(labels, ids, row_offset, small_rank, lo, hi, n_labels, votes=None):
    """stego_regions_votes -> votes int32 [hi - lo, n_labels] (reset by the call)."""
    _require_dev(labels, ids, row_offset, small_rank, votes)
    desc = _regions_desc_of(labels, 4)
    _expect("regions", "ids", ids, torch.int32, labels.shape)
    _expect("regions", "small_rank", small_rank, torch.int32, (small_rank.numel(),))
    rows = max(int(hi) - int(lo), 0)
    if votes is None:
        votes = torch.empty((rows, max(int(n_labels), 0)), dtype=torch.int32, device=labels.device)
    elif votes.dtype != torch.int32 or votes.numel() < rows * int(n_labels) or not votes.is_contiguous():
        raise RuntimeError("regions: votes must be a contiguous int32 tensor of at least (hi - lo) * n_labels elements")
    with _on_device(labels.device):
        _check(regions_votes_raw(desc, labels, ids, row_offset, small_rank.numel(), small_rank, lo, hi, n_labels, votes, _stream()))
    return votes


def regions_relabel(labels_in, labels_out, ids, row_offset, small_rank, first, lo, hi, n_labels, votes, changed):
    """stego_regions_relabel: the small regions of ranks [lo, hi) rewritten in labels_out, changed int32 [1] += the regions that changed."""
    _require_dev(labels_in, labels_out, ids, row_offset, small_rank, first, votes, changed)
    desc = _regions_desc_of(labels_in, 4)
    if labels_out.dtype != labels_in.dtype or labels_out.shape != labels_in.shape or not labels_out.is_contiguous() or \
            labels_out.data_ptr() == labels_in.data_ptr():
        raise RuntimeError("regions: labels_out must be another contiguous tensor of labels_in's dtype and shape")
    _expect("regions", "ids", ids, torch.int32, labels_in.shape)
    _expect("regions", "small_rank", small_rank, torch.int32, (small_rank.numel(),))
    _expect("regions", "first", first, torch.int32, (small_rank.numel(),))
    _expect("regions", "changed", changed, torch.int32, (1,))
    if votes.dtype != torch.int32 or votes.numel() < max(int(hi) - int(lo), 0) * int(n_labels) or not votes.is_contiguous():
        raise RuntimeError("regions: votes must be a contiguous int32 tensor of at least (hi - lo) * n_labels elements")
    with _on_device(labels_in.device):
        _check(regions_relabel_raw(desc, labels_in, labels_out, ids, row_offset, small_rank.numel(), small_rank, first, lo, hi, n_labels,
                                   votes, changed, _stream()))


# ---- region descriptors (include/stego_region_pool.h; stego_amd.region_descriptors wraps them)
region_pool_desc = _desc(StegoRegionPoolDesc)
region_pool_workspace_bytes = _bytes("stego_region_pool_workspace_bytes")
region_pool_raw = _raw("stego_region_pool")


def region_pool_plan(desc):
    """stego_region_pool_plan (host only) -> (return code, segment length in pixels, channel block, [(LDS bytes, workgroups) of the
    range, pool and finish launches])."""
    seg, cb = c_int32(-1), c_int32(-1)
    lds, wgs = (c_size_t * REGION_POOL_LAUNCHES)(), (c_int64 * REGION_POOL_LAUNCHES)()
    rc = load().stego_region_pool_plan(byref(desc), byref(seg), byref(cb), lds, wgs)
    return int(rc), int(seg.value), int(cb.value), [(int(a), int(b)) for a, b in zip(lds, wgs)]


def region_pool(maps, ids, row_offset, area, lo, hi, out=None, workspace=None):
    """stego_region_pool on torch's current stream, nothing synchronised: maps float32 [B, C, h, w] (any strides), ids int32 [B, H, W],
    row_offset int64 [B], area int32 [capacity] -> float32 [hi - lo, C], the descriptors of the table rows [lo, hi).  `out` and
    `workspace` (uint8, from an earlier call of at least as many rows) are reused when given."""
    _require_dev(maps, ids, row_offset, area, out, workspace)
    m = _map(maps)
    _expect("region_pool", "ids", ids, torch.int32, (maps.shape[0], None, None))
    _expect("region_pool", "row_offset", row_offset, torch.int64, (maps.shape[0],))
    _expect("region_pool", "area", area, torch.int32, (None,))
    B, C, h, w = maps.shape
    rows = max(int(hi) - int(lo), 0)
    desc = region_pool_desc(B, C, h, w, ids.shape[1], ids.shape[2], rows)
    need = _workspace_need(region_pool_workspace_bytes, desc, lambda: _call("stego_region_pool_plan", desc, None, None, None, None))
    dev = maps.device
    if out is None:
        out = torch.empty((rows, C), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.numel() < rows * C or not out.is_contiguous():
        raise RuntimeError("region_pool: out must be a contiguous float32 tensor of at least (hi - lo) * C elements")
    if workspace is None or workspace.numel() < need:
        workspace = _empty_bytes(need, dev)
    with _on_device(dev):
        _check(region_pool_raw(desc, m, ids, row_offset, area, area.numel(), lo, hi, out, workspace, workspace.numel(), _stream()))
    return out


# ---- device-side confusion matrices (include/stego_confusion.h; stego_amd.metrics wraps them for the trainer and evaluate())
probe_confusion_desc = _desc(StegoProbeConfusionDesc)
confusion_desc = _desc(StegoConfusionDesc)
probe_confusion_raw = _raw("stego_probe_confusion")
confusion_raw = _raw("stego_confusion")


def probe_confusion_plan(desc):
    """stego_probe_confusion_plan (host only) -> (LDS bytes, histograms included; tile rows; tile columns); 0 bytes for an invalid
    descriptor."""
    ty, tx = c_int32(0), c_int32(0)
    n = load().stego_probe_confusion_plan(byref(desc), byref(ty), byref(tx))
    return int(n), ty.value, tx.value


def _counts_ok(counts, n, n_classes, name):
    if counts.dtype != torch.int64 or tuple(counts.shape) != (n, n_classes) or not counts.is_contiguous():
        raise ValueError("%s: expected a contiguous int64 [%d, %d] tensor, got %s %s" % (name, n, n_classes, counts.dtype, tuple(counts.shape)))


def probe_confusion(code, code_flip, lin_w, lin_b, centroids, labels, lin_counts, clu_counts, alpha):
    """stego_probe_confusion: code (and code_flip, or None) float32 [B, K, h, w] with any strides, labels int64 [B, H, W], and per
    probe its weights (lin_w [n_lin, K] and lin_b [n_lin]; centroids [n_clu, K], L2-normalised) and its int64 [n, n_classes] matrix,
    which is added onto in place.  A probe whose counts are None is skipped; n_classes is the counts' second dimension.  Nothing is
    returned and nothing synchronises."""
    if lin_counts is None and clu_counts is None:
        raise ValueError("probe_confusion: both probes skipped")
    _require_dev(code, code_flip, labels, lin_counts, clu_counts)
    B, K, h, w = code.shape
    if labels.dtype != torch.int64 or labels.dim() != 3 or labels.shape[0] != B:
        raise ValueError("labels: expected int64 [%d, H, W], got %s %s" % (B, labels.dtype, tuple(labels.shape)))
    if code_flip is not None and tuple(code_flip.shape) != tuple(code.shape):
        raise ValueError("code_flip %s does not match code %s" % (tuple(code_flip.shape), tuple(code.shape)))
    H, W = int(labels.shape[1]), int(labels.shape[2])
    n_classes = int((lin_counts if lin_counts is not None else clu_counts).shape[1])
    lw = lb = ce = None
    n_lin = n_clu = 0
    if lin_counts is not None:
        _require_dev(lin_w, lin_b)
        lw, lb = _dense(lin_w, torch.float32), _dense(lin_b, torch.float32)
        n_lin = int(lw.shape[0])
        if tuple(lw.shape) != (n_lin, K) or tuple(lb.shape) != (n_lin,):
            raise ValueError("linear probe weights %s / %s do not match K = %d" % (tuple(lw.shape), tuple(lb.shape), K))
        _counts_ok(lin_counts, n_lin, n_classes, "lin_counts")
    if clu_counts is not None:
        _require_dev(centroids)
        ce = _dense(centroids, torch.float32)
        n_clu = int(ce.shape[0])
        if tuple(ce.shape) != (n_clu, K):
            raise ValueError("centroids %s do not match K = %d" % (tuple(ce.shape), K))
        _counts_ok(clu_counts, n_clu, n_classes, "clu_counts")
    labels = labels.contiguous()
    desc = probe_confusion_desc(B, K, h, w, H, W, n_lin, n_clu, lin_counts is not None, clu_counts is not None, alpha, n_classes)
    with _on_device(code.device):
        _check(probe_confusion_raw(desc, _map(code), _map(code_flip) if code_flip is not None else None, lw, lb, ce, labels,
                                   lin_counts, clu_counts, _stream()))


def confusion(pred, labels, counts, kind):
    """stego_confusion: `pred` is int64 [B, H, W] label maps (kind "labels") or float32 [B, n, H, W] scores (kind "scores": the
    prediction is the first maximum over n), labels int64 [B, H, W]; counts int64 [n, n_classes] is added onto in place.  Nothing is
    returned and nothing synchronises."""
    if kind not in CONF_KINDS:
        raise ValueError("confusion: kinds are %s, got %r" % (sorted(CONF_KINDS), kind))
    _require_dev(pred, labels, counts)
    if counts.dtype != torch.int64 or counts.dim() != 2 or not counts.is_contiguous():
        raise ValueError("counts: expected a contiguous int64 [n, n_classes] tensor, got %s %s" % (counts.dtype, tuple(counts.shape)))
    n, n_classes = int(counts.shape[0]), int(counts.shape[1])
    if labels.dtype != torch.int64 or labels.dim() != 3:
        raise ValueError("labels: expected int64 [B, H, W], got %s %s" % (labels.dtype, tuple(labels.shape)))
    B, H, W = labels.shape
    if kind == "scores":
        if pred.dtype != torch.float32 or tuple(pred.shape) != (B, n, H, W):
            raise ValueError("scores: expected float32 %s, got %s %s" % ((B, n, H, W), pred.dtype, tuple(pred.shape)))
    elif pred.dtype != torch.int64 or tuple(pred.shape) != (B, H, W):
        raise ValueError("label maps: expected int64 %s, got %s %s" % ((B, H, W), pred.dtype, tuple(pred.shape)))
    pred, labels = pred.contiguous(), labels.contiguous()
    desc = confusion_desc(B, n, H, W, n_classes, CONF_KINDS[kind])
    with _on_device(labels.device):
        _check(confusion_raw(desc, pred, labels, counts, _stream()))


# ---- fused Adam step (include/stego_optim.h; stego_amd.optim.FusedAdam wraps it for the trainer)
def adam_segments(records):
    """The host copy of the segment table: (param address, count, grad_offset, state_offset, group) per record -> a ctypes array."""
    table = (StegoAdamSegment * max(len(records), 1))()
    for r, (addr, count, grad_offset, state_offset, group) in zip(table, records):
        r.param, r.count, r.grad_offset, r.state_offset, r.group = addr, int(count), int(grad_offset), int(state_offset), int(group)
    return table


def adam_desc(n_segments, groups, zero_grads, grad_elems, state_elems, n_groups=None):
    """`groups`: (lr, beta1, beta2, eps[, active]) per group, at most ADAM_MAX_GROUPS of them."""
    d = StegoAdamDesc(int(n_segments), len(groups) if n_groups is None else int(n_groups), int(zero_grads), 0, int(grad_elems),
                      int(state_elems))
    for g, vals in zip(d.groups, groups):
        g.lr, g.beta1, g.beta2, g.eps = (float(x) for x in vals[:4])
        g.active = int(vals[4]) if len(vals) > 4 else 1
    return d


def adam_plan(desc, segments_host):
    """stego_adam_plan (host only) -> (return code, grid, chunk, n_chunks); the last three are 0 when the code is not 0."""
    grid, chunk, n = c_int32(0), c_int32(0), c_int64(0)
    rc = _call("stego_adam_plan", desc, segments_host, byref(grid), byref(chunk), byref(n))
    return rc, grid.value, chunk.value, n.value


adam_step_raw = _raw("stego_adam_step")       # (`segments_host`: the ctypes array of adam_segments, or None)


def adam_step(desc, segments_host, segments, grads, exp_avg, exp_avg_sq, steps, ticket):
    """stego_adam_step on torch's current stream: `segments` is the device copy of `segments_host` (a uint8 tensor), grads / exp_avg /
    exp_avg_sq flat float32 tensors, steps int32 [n_groups], ticket int32 [1] (zero before the first call).  One launch; nothing is
    returned and nothing synchronises."""
    _require_dev(segments, grads, exp_avg, exp_avg_sq, steps, ticket)
    with _on_device(grads.device):
        _check(adam_step_raw(desc, segments_host, segments, grads, exp_avg, exp_avg_sq, steps, ticket, _stream()))


# ---- device-side step statistics (include/stego_stats.h; stego_amd.step_stats.StepStats wraps them for the trainer)
def stats_desc(counts, n_scalars, with_hist, ring_slots, n_tensors=None):
    d = StegoStatsDesc(len(counts) if n_tensors is None else int(n_tensors), int(n_scalars), int(with_hist), int(ring_slots))
    for i, c in enumerate(list(counts)[:STATS_MAX_TENSORS]):
        d.counts[i] = int(c)
    return d


def step_stats_plan(desc):
    """stego_step_stats_plan (host only) -> (return code, {field: value}); the dict is empty when the code is not 0."""
    plan = StegoStatsPlan()
    rc = _call("stego_step_stats_plan", desc, plan)
    return rc, ({name: int(getattr(plan, name)) for name in STATS_PLAN_FIELDS} if rc == 0 else {})


def step_stats_edges():
    """stego_step_stats_edges (host only) -> (limits float64 [1549], thresholds float32 [1549]) as numpy arrays."""
    import numpy as np
    limits, thr = np.empty(STATS_LIMITS, np.float64), np.empty(STATS_LIMITS, np.float32)
    _check(load().stego_step_stats_edges(limits.ctypes.data, thr.ctypes.data))
    return limits, thr


def step_stats_raw(desc, tensors, scalars, ring, state, workspace, stream=None):
    """stego_step_stats with every argument given: `tensors` / `scalars` lists of tensors or raw addresses (or None for a NULL array),
    the rest raw addresses or tensors (tests: the error codes) -> the return code, unchecked."""
    def table(xs):
        if xs is None:
            return None
        arr = (c_void_p * max(len(xs), 1))()
        for i, x in enumerate(xs):
            arr[i] = _addr(x)
        return arr
    return _call("stego_step_stats", desc, table(tensors), table(scalars), ring, state, workspace, stream)


def pointer_table(n):
    """A host array of n device addresses (stego_step_stats's `tensors` / `scalars`), to be filled in place."""
    return (c_void_p * max(int(n), 1))()


def step_stats_call(desc, tensor_table, scalar_table, addresses, device):
    """stego_step_stats on torch's current stream from tables the caller keeps (stego_amd.step_stats.StepStats: once per training
    step): `addresses` = (ring, state, workspace) as integers."""
    with _on_device(device):
        _check(load().stego_step_stats(byref(desc), tensor_table, scalar_table, addresses[0], addresses[1], addresses[2], _stream()))


def step_stats(desc, tensors, scalars, ring, state, workspace):
    """stego_step_stats on torch's current stream: one launch; nothing is returned and nothing synchronises."""
    _require_dev(ring, state, workspace, *tensors)
    _require_dev(*scalars)
    with _on_device(ring.device):
        _check(step_stats_raw(desc, tensors, scalars, ring, state, workspace, _stream()))


# ---- fused training tail of the two probes (include/stego_probe_train.h; stego_amd.probe_train wraps it for the trainer)
probe_train_desc = _desc(StegoProbeTrainDesc)
probe_train_workspace_bytes = _bytes("stego_probe_train_workspace_bytes")
probe_train_raw = _raw("stego_probe_train")


def probe_train_plan(desc):
    """stego_probe_train_plan (host only) -> (LDS bytes per workgroup, workgroups of the main kernel); 0 bytes for an invalid descriptor."""
    wgs = c_int32(0)
    n = load().stego_probe_train_plan(byref(desc), byref(wgs))
    return int(n), wgs.value


def probe_train(code, label, lin_w, lin_b, clusters):
    """stego_probe_train: code float32 [B, K, h, w] with any strides, label int64 [B, H, W], lin_w [n_lin, K], lin_b [n_lin], clusters
    [n_clu, K] (not normalised) on one HIP device -> (losses float32 [2] (linear, cluster), n_valid int64 [1], d_lin_w, d_lin_b,
    d_clusters).  A probe whose weights are None is skipped: its loss slot stays 0 and its gradients are None."""
    _require_dev(code, label, lin_w, lin_b, clusters)
    B, K, h, w = code.shape
    lin, clu = lin_w is not None, clusters is not None
    dev = code.device
    n_lin = int(lin_w.shape[0]) if lin else 0
    n_clu = int(clusters.shape[0]) if clu else 0
    if lin:
        if label.dtype != torch.int64 or label.dim() != 3 or label.shape[0] != B:
            raise ValueError("probe_train expects an int64 [B, H, W] label map, got %s %s" % (label.dtype, tuple(label.shape)))
        label = _dense(label, torch.int64)
        H, W = int(label.shape[1]), int(label.shape[2])
        lin_w, lin_b = _dense(lin_w.reshape(n_lin, -1), torch.float32), _dense(lin_b, torch.float32)
        if tuple(lin_w.shape) != (n_lin, K) or tuple(lin_b.shape) != (n_lin,):
            raise ValueError("linear probe %s / %s does not match K = %d" % (tuple(lin_w.shape), tuple(lin_b.shape), K))
    else:
        H, W, label = h, w, None
    if clu:
        clusters = _dense(clusters, torch.float32)
        if tuple(clusters.shape) != (n_clu, K):
            raise ValueError("clusters %s do not match K = %d" % (tuple(clusters.shape), K))
    desc = probe_train_desc(B, K, h, w, H, W, n_lin, n_clu)
    losses = torch.zeros(2, dtype=torch.float32, device=dev)
    n_valid = torch.empty(1, dtype=torch.int64, device=dev)
    d_lin_w = torch.empty(n_lin, K, dtype=torch.float32, device=dev) if lin else None
    d_lin_b = torch.empty(n_lin, dtype=torch.float32, device=dev) if lin else None
    d_clusters = torch.empty(n_clu, K, dtype=torch.float32, device=dev) if clu else None
    mc = _map(code)
    ws, n = _workspace(probe_train_workspace_bytes, desc, dev, lambda: probe_train_raw(
        desc, mc, label, lin_w, lin_b, clusters, losses, n_valid, d_lin_w, d_lin_b, d_clusters, None, 0))
    with _on_device(dev):
        _check(probe_train_raw(desc, mc, label, lin_w, lin_b, clusters, losses, n_valid, d_lin_w, d_lin_b, d_clusters, ws, n, _stream()))
    return losses, n_valid, d_lin_w, d_lin_b, d_clusters


# ---- label co-occurrence PR histogram of feature correspondences (include/stego_pr.h; stego_amd.correspondence_pr wraps it)
pr_desc = _desc(StegoPrDesc, flags=0)
pr_accumulate_raw = _raw("stego_pr_accumulate")


def pr_plan(desc):
    """stego_pr_plan (host only) -> (LDS bytes, point tiles of coords1, point tiles of coords2); 0 bytes for an invalid descriptor."""
    t1, t2 = c_int32(0), c_int32(0)
    n = load().stego_pr_plan(byref(desc), byref(t1), byref(t2))
    return int(n), t1.value, t2.value


def pr_accumulate(a, b, labels_a, labels_b, coords1, coords2, hist, n_classes, index_b=None, normalize=True, skip_unlabeled=False):
    """stego_pr_accumulate: a, b float32 [B, C, h, w] (any strides), labels_a / labels_b integer [B, HL, WL], coords1 [B, N1, 2] or
    [B, S, S, 2] and coords2 likewise, hist int64 [n_bins, 2] (negatives, positives), all on one HIP device.  Adds every pair
    (point of coords1, point of coords2) of every image to `hist` in place and returns it; image i of `a` is paired with image
    index_b[i] of `b` / `labels_b` (i itself without index_b)."""
    _require_dev(a, b, labels_a, labels_b, coords1, coords2, hist, index_b)
    if a.dim() != 4 or tuple(a.shape) != tuple(b.shape):
        raise ValueError("pr_accumulate expects two float32 maps of one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    B, C, h, w = a.shape
    if labels_a.dim() != 3 or tuple(labels_a.shape) != tuple(labels_b.shape) or labels_a.shape[0] != B:
        raise ValueError("pr_accumulate expects two [B, HL, WL] label maps, got %s and %s" % (tuple(labels_a.shape), tuple(labels_b.shape)))
    if hist.dtype != torch.int64 or hist.dim() != 2 or hist.shape[1] != 2 or not hist.is_contiguous():
        raise ValueError("pr_accumulate expects a contiguous int64 [n_bins, 2] histogram")
    c1 = _dense(coords1.reshape(B, -1, 2), torch.float32)
    c2 = _dense(coords2.reshape(B, -1, 2), torch.float32)
    la, lb = _dense(labels_a, torch.int64), _dense(labels_b, torch.int64)
    if index_b is not None:
        index_b = _dense(index_b, torch.int64)
        if index_b.numel() != B:
            raise ValueError("index_b has %d entries for %d images" % (index_b.numel(), B))
    flags = (0 if normalize else PR_RAW) | (PR_SKIP_UNLABELED if skip_unlabeled else 0)
    desc = pr_desc(B, C, h, w, la.shape[1], la.shape[2], c1.shape[1], c2.shape[1], hist.shape[0], n_classes, flags)
    with _on_device(a.device):
        _check(pr_accumulate_raw(desc, _map(a), _map(b), la, lb, index_b, c1, c2, hist, _stream()))
    return hist


# ---- query-point correspondence heatmaps (include/stego_heat.h; stego_amd.correspondence_heatmaps wraps it)
heat_desc = _desc(StegoHeatDesc, flags=0)
heat_workspace_bytes = _bytes("stego_heat_workspace_bytes")
corr_heatmaps_raw = _raw("stego_corr_heatmaps")


def heat_plan(desc):
    """stego_heat_plan (host only) -> (LDS bytes of the first launch, its grid, the second launch's grid, its LDS bytes, its output
    rows per workgroup); 0 bytes for an invalid descriptor."""
    g1, g2, lds2, rows = (c_int32 * 3)(), (c_int32 * 3)(), c_size_t(0), c_int32(0)
    n = load().stego_heat_plan(byref(desc), g1, g2, byref(lds2), byref(rows))
    return int(n), tuple(g1), tuple(g2), int(lds2.value), rows.value


def heat_workspace_views(desc, ws):
    """The four arrays of the workspace of a finished call (include/stego_heat.h) as views of the uint8 tensor `ws`:
    psum float64 [B, N, NCH], low float32 [B, N, h, w], pmax float32 [B, N, NCH], pidx int32 [B, N, NCH]."""
    rows, hw = desc.B * desc.N, desc.h * desc.w
    nch = -(-hw // 128)
    o1 = rows * nch * 8
    o2 = o1 + rows * hw * 4
    o3 = o2 + rows * nch * 4
    return (ws[:o1].view(torch.float64).view(desc.B, desc.N, nch), ws[o1:o2].view(torch.float32).view(desc.B, desc.N, desc.h, desc.w),
            ws[o2:o3].view(torch.float32).view(desc.B, desc.N, nch), ws[o3:o3 + rows * nch * 4].view(torch.int32).view(desc.B, desc.N, nch))


def corr_heatmaps(src, tgt, points, size, center=True, clamp=True, index_t=None, want_best=False, keep_workspace=False):
    """stego_corr_heatmaps: src float32 [B, C, hs, ws], tgt float32 [B, C, h, w] (any strides), points [B, N, 2] or [B, N, 1, 2] as
    (x, y) in [-1, 1], index_t int64 [B] or None, all on one HIP device -> heat float32 [B, N, H, W] for size = (H, W); with want_best
    also peak [B, N] and best [B, N, 2]; with keep_workspace also (desc, workspace) for capi.heat_workspace_views."""
    _require_dev(src, tgt, points, index_t)
    if src.dim() != 4 or tgt.dim() != 4 or src.shape[:2] != tgt.shape[:2]:
        raise ValueError("corr_heatmaps expects two float32 maps [B, C, ., .] of one B and C, got %s and %s" % (tuple(src.shape), tuple(tgt.shape)))
    B, C, hs, ws_ = src.shape
    h, w = int(tgt.shape[2]), int(tgt.shape[3])
    if points.shape[0] != B or points.shape[-1] != 2:
        raise ValueError("corr_heatmaps expects points [B, N, 2] or [B, N, 1, 2], got %s" % (tuple(points.shape),))
    pts = _dense(points.reshape(B, -1, 2), torch.float32)
    N = int(pts.shape[1])
    H, W = int(size[0]), int(size[1])
    if index_t is not None:
        index_t = _dense(index_t, torch.int64)
        if index_t.numel() != B:
            raise ValueError("index_t has %d entries for %d images" % (index_t.numel(), B))
    desc = heat_desc(B, C, hs, ws_, h, w, N, H, W, (0 if center else HEAT_NO_CENTER) | (0 if clamp else HEAT_NO_CLAMP))
    dev = src.device
    ms, mt = _map(src), _map(tgt)
    ws, n = _workspace(heat_workspace_bytes, desc, dev, lambda: corr_heatmaps_raw(desc, ms, mt, index_t, pts, 16, None, None, None, 0))
    heat = torch.empty(B, N, H, W, dtype=torch.float32, device=dev)
    peak = torch.empty(B, N, dtype=torch.float32, device=dev) if want_best else None
    best = torch.empty(B, N, 2, dtype=torch.float32, device=dev) if want_best else None
    with _on_device(dev):
        _check(corr_heatmaps_raw(desc, ms, mt, index_t, pts, heat, peak, best, ws, n, _stream()))
    out = (heat, peak, best) if want_best else heat
    if keep_workspace:
        return out, desc, ws
    return out


# ---- fused ContrastiveCRFLoss, forward and backward (include/stego_crf_loss.h; stego_amd.crf_loss wraps it for the trainer)
crf_loss_desc = _desc(StegoCrfLossDesc, flags=CRFLOSS_NORMALIZE)
crf_loss_workspace_bytes = _bytes("stego_crf_loss_workspace_bytes")
crf_loss_raw = _raw("stego_crf_loss")


def crf_loss_plan(desc):
    """stego_crf_loss_plan (host only) -> (return code, [(LDS bytes, workgroups) of the prepare, pairs and finish launch])."""
    return _launch_plan("stego_crf_loss_plan", desc, CRFLOSS_LAUNCHES)


def crf_loss(guidance, code, coords, size, params, normalize=True, need_grad=True, want_per_image=True, d_code_like=None):
    """stego_crf_loss: guidance float32 [B, G, hg, wg], code float32 [B, K, h, w] (any strides), coords int64 [2, N] (rows, columns) on
    the grid size = (H, W), params = (alpha, beta, gamma, w1, w2, shift), all on one HIP device -> (loss float32 [1], per_image
    float32 [B] or None, d_code float32 [B, K, h, w] for a unit upstream or None).  d_code takes the memory layout of `d_code_like`
    (default: of the code).  The workspace comes from torch's caching allocator, as for the other fused calls."""
    _require_dev(guidance, code, coords)
    if guidance.dim() != 4 or code.dim() != 4 or guidance.shape[0] != code.shape[0]:
        raise ValueError("crf_loss expects a guidance [B, G, ., .] and a code [B, K, ., .], got %s and %s"
                         % (tuple(guidance.shape), tuple(code.shape)))
    if coords.dim() != 2 or coords.shape[0] != 2:
        raise ValueError("crf_loss expects coords [2, N], got %s" % (tuple(coords.shape),))
    B, K, h, w = code.shape
    G, hg, wg = guidance.shape[1:]
    coords = _dense(coords, torch.int64)
    dev = code.device
    desc = crf_loss_desc(B, K, G, h, w, hg, wg, size[0], size[1], coords.shape[1], *params, CRFLOSS_NORMALIZE if normalize else 0)
    mg, mc = _map(guidance), _map(code)
    ws, n = _workspace(crf_loss_workspace_bytes, desc, dev, lambda: _call("stego_crf_loss_plan", desc, None, None))
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    per_image = torch.empty(B, dtype=torch.float32, device=dev) if want_per_image else None
    d_code = torch.empty_like(code if d_code_like is None else d_code_like, dtype=torch.float32) if need_grad else None
    with _on_device(dev):
        _check(crf_loss_raw(desc, mg, mc, coords, loss, per_image, _map(d_code) if need_grad else None, ws, n, _stream()))
    return loss, per_image, d_code


# ---- device-side augmented views and the fused aug-alignment loss (include/stego_aug.h; stego_amd.augment wraps them for the trainer)
aug_desc = _desc(StegoAugDesc)
augment_workspace_bytes = _bytes("stego_augment_workspace_bytes")
augment_raw = _raw("stego_augment")       # (`params_host`: a ctypes array of StegoAugParams, a raw address or None)
aug_align_desc = _desc(StegoAugAlignDesc)
aug_align_workspace_bytes = _bytes("stego_aug_align_workspace_bytes")
aug_align_raw = _raw("stego_aug_align")


def aug_check_params(desc, records):
    """stego_augment_check_params (host only): `records` a ctypes array of StegoAugParams (or None) ->
    (return code, index of the first bad record or -1, whether a record applies contrast)."""
    bad, contrast = c_int64(-1), c_int32(0)
    rc = _call("stego_augment_check_params", desc, records, byref(bad), byref(contrast))
    return rc, int(bad.value), bool(contrast.value)


def augment_plan(desc):
    """stego_augment_plan (host only) -> (return code, [(LDS bytes, workgroups) of the mean and the apply launch])."""
    return _launch_plan("stego_augment_plan", desc, AUG_LAUNCHES)


def aug_table(records, dev):
    """The B records as device bytes: one small copy from pinned memory on the current stream; nothing waits for the device."""
    host = torch.frombuffer(bytearray(bytes(records)), dtype=torch.uint8).pin_memory()
    return host.to(dev, non_blocking=True)


def augment(img, records, R, table=None):
    """stego_augment: img float32 [B, 3, H, W] on a HIP device (any strides), `records` a ctypes array of B StegoAugParams ->
    (img_aug float32 [B, 3, R, R], coord_aug float32 [B, R, R, 2]).  `table`: aug_table(records, device) made earlier (a call that
    is captured into a graph takes it from outside the capture); by default it is made here."""
    _require_dev(img)
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError("augment expects an image batch [B, 3, H, W], got %s" % (tuple(img.shape),))
    B, _, H, W = img.shape
    if len(records) != B:
        raise ValueError("augment: %d parameter records for %d images" % (len(records), B))
    dev = img.device
    desc = aug_desc(B, H, W, R)
    m = _map(img)
    ws, n = _workspace(augment_workspace_bytes, desc, dev, lambda: _call("stego_augment_plan", desc, None, None))
    img_aug = torch.empty(B, 3, R, R, dtype=torch.float32, device=dev)
    coord_aug = torch.empty(B, R, R, 2, dtype=torch.float32, device=dev)
    with _on_device(dev):
        if table is None:
            table = aug_table(records, dev)
        _check(augment_raw(desc, m, records, table, img_aug, coord_aug, ws, n, _stream()))
    return img_aug, coord_aug


def aug_align_plan(desc):
    """stego_aug_align_plan (host only) -> (return code, [(LDS bytes, workgroups) of the pixels and the finish launch])."""
    return _launch_plan("stego_aug_align_plan", desc, AUGALIGN_LAUNCHES)


def aug_align(code, code_aug, coord, need_code=True, need_code_aug=True):
    """stego_aug_align: code float32 [B, K, h, w] and code_aug float32 [B, K, S, S] (any strides), coord float32 [B, Rh, Rw, 2], all
    on one HIP device -> (loss float32 [1], d_code or None, d_code_aug or None), the gradients for a unit upstream in the layout of
    their inputs.  The workspace comes from torch's caching allocator, as for the other fused calls."""
    _require_dev(code, code_aug, coord)
    if code.dim() != 4 or code_aug.dim() != 4 or code_aug.shape[:2] != code.shape[:2] or code_aug.shape[2] != code_aug.shape[3]:
        raise ValueError("aug_align expects a code [B, K, h, w] and a square code_aug [B, K, S, S], got %s and %s"
                         % (tuple(code.shape), tuple(code_aug.shape)))
    if coord.dim() != 4 or coord.shape[0] != code.shape[0] or coord.shape[3] != 2:
        raise ValueError("aug_align expects coord [B, Rh, Rw, 2], got %s" % (tuple(coord.shape),))
    B, K, h, w = code.shape
    coord = _dense(coord, torch.float32)
    dev = code.device
    desc = aug_align_desc(B, K, h, w, code_aug.shape[2], coord.shape[1], coord.shape[2])
    mc, ma = _map(code), _map(code_aug)
    ws, n = _workspace(aug_align_workspace_bytes, desc, dev, lambda: _call("stego_aug_align_plan", desc, None, None))
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    d_code = torch.empty_like(code) if need_code else None
    d_code_aug = torch.empty_like(code_aug) if need_code_aug else None
    with _on_device(dev):
        _check(aug_align_raw(desc, mc, ma, coord, loss, _map(d_code) if need_code else None,
                             _map(d_code_aug) if need_code_aug else None, ws, n, _stream()))
    return loss, d_code, d_code_aug


# ---- fused reconstruction loss, forward and backward (include/stego_rec.h; stego_amd.rec_loss wraps it for the trainer)
rec_desc = _desc(StegoRecDesc)
rec_loss_workspace_bytes = _bytes("stego_rec_loss_workspace_bytes")
rec_loss_raw = _raw("stego_rec_loss")


def rec_loss_plan(desc):
    """stego_rec_loss_plan (host only) -> (return code, [(LDS bytes, workgroups) of the tiles and the finish launch])."""
    return _launch_plan("stego_rec_loss_plan", desc, REC_LAUNCHES)


def rec_loss(code, feats, weight, bias, need_code=True, need_weight=True, need_bias=True):
    """stego_rec_loss: code float32 [B, K, h, w] and feats float32 [B, C, h, w] (any strides), weight [C, K] (or the convolution's
    [C, K, 1, 1]) and bias [C], all on one HIP device -> (loss float32 [1], d_code, d_weight, d_bias; None where not asked for), the
    gradients for a unit upstream, d_code in the layout of `code`, d_weight in the shape of `weight`.  The workspace comes from torch's
    caching allocator, as for the other fused calls."""
    _require_dev(code, feats, weight, bias)
    if code.dim() != 4 or feats.dim() != 4 or feats.shape[0] != code.shape[0] or feats.shape[2:] != code.shape[2:]:
        raise ValueError("rec_loss expects a code [B, K, h, w] and feats [B, C, h, w], got %s and %s" % (tuple(code.shape), tuple(feats.shape)))
    B, K, h, w = code.shape
    C = feats.shape[1]
    if weight.numel() != C * K or weight.shape[:2] != (C, K) or tuple(bias.shape) != (C,):
        raise ValueError("rec_loss expects a weight [%d, %d] and a bias [%d], got %s and %s" % (C, K, C, tuple(weight.shape), tuple(bias.shape)))
    weight, bias = _dense(weight, torch.float32), _dense(bias, torch.float32)
    dev = code.device
    desc = rec_desc(B, K, C, h, w)
    mc, mf = _map(code), _map(feats)
    ws, n = _workspace(rec_loss_workspace_bytes, desc, dev, lambda: _call("stego_rec_loss_plan", desc, None, None))
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    d_code = torch.empty_like(code) if need_code else None
    d_weight = torch.empty_like(weight) if need_weight else None
    d_bias = torch.empty_like(bias) if need_bias else None
    with _on_device(dev):
        _check(rec_loss_raw(desc, mc, mf, weight, bias, loss, _map(d_code) if need_code else None, d_weight, d_bias, ws, n, _stream()))
    return loss, d_code, d_weight, d_bias
