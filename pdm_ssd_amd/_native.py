"""ctypes binding of libpdmssd_hip.so (the C ABI declared in include/pdmssd_hip.h).

There is deliberately NO fallback: if the HIP library is missing or a call fails, an exception is
raised.  Nothing here imports the CPU oracle.
"""
import ctypes
import os
import re

# torch first: its wheel bundles the HIP runtime (libamdhip64.so.7) this library must share with it —
# streams and device pointers handed across the C ABI are only meaningful inside ONE runtime instance.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpdmssd_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "pdmssd_hip.h")
ABI_VERSION = 1

_lib = None

_declared = None    # name -> (restype, argtypes), parsed from the header on the first lib()

_CTYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
           "long long": ctypes.c_longlong, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint,
           "unsigned long long": ctypes.c_ulonglong}
_RESTYPES = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p}


class NativeLibraryError(RuntimeError):
    pass


def _param_ctype(name, param):
    if "*" in param:
        return ctypes.c_void_p
    words = [w for w in param.split() if w != "const"]
    for typ in (" ".join(words), " ".join(words[:-1])):     # unnamed, or with the parameter's name last
        if typ in _CTYPES:
            return _CTYPES[typ]
    raise NativeLibraryError(f"{name}: parameter `{param.strip()}` has a type the binding does not know")


def parse_header(text):
    """Every `ret pdm_name(params);` prototype of a C header -> {name: (restype, [argtypes])}.  Pointers of any kind become
    c_void_p; a type outside _CTYPES / _RESTYPES raises instead of being guessed."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*|^[ \t]*#.*$", " ", text, flags=re.M)
    out = {}
    for stmt in re.split(r"[;{}]", text):
        if not re.search(r"\bpdm_\w+\s*\(", stmt):
            continue
        m = re.fullmatch(r"\s*(.*?)\b(pdm_\w+)\s*\(([^()]*)\)\s*", stmt, flags=re.S)
        if not m:
            raise NativeLibraryError(f"cannot parse the prototype `{' '.join(stmt.split())}`")
        ret, name, params = m.groups()
        ret = " ".join(ret.replace("*", " * ").split())
        if ret not in _RESTYPES:
            raise NativeLibraryError(f"{name}: return type `{ret}` is one the binding does not know")
        params = [] if params.strip() in ("", "void") else params.split(",")
        out[name] = (_RESTYPES[ret], [_param_ctype(name, p) for p in params])
    return out


def declared():
    """The ABI as include/pdmssd_hip.h declares it (parsed once)."""
    global _declared
    if _declared is None:
        try:
            with open(HEADER_PATH) as f:
                text = f.read()
        except OSError as e:
            raise NativeLibraryError(f"{HEADER_PATH}: the header that describes libpdmssd_hip.so cannot be read ({e})")
        _declared = parse_header(text)
    return _declared


def __getattr__(name):
    if name == "EXPORTS":       # the declared names; read from the header when first asked for, not at import
        return list(declared())
    raise AttributeError(name)


def lib():
    """Load libpdmssd_hip.so once; raise loudly when it is absent (no CPU fallback exists).  Every function the header
    declares gets its restype and argtypes from there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                f"{LIB_PATH} not found: build it with `make -C pdm_ssd_amd/csrc` "
                "(or `python -c 'import __graft_entry__ as g; g.build()'`). "
                "pdm_ssd_amd has no CPU or PyTorch fallback for its operators.")
        l = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in declared().items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = restype, argtypes
        if l.pdm_abi_version() != ABI_VERSION:
            raise NativeLibraryError(
                f"libpdmssd_hip.so ABI {l.pdm_abi_version()} != expected {ABI_VERSION}; rebuild it")
        _lib = l
    return _lib


def call(name, stream, *args):
    """Invoke an entry point on `stream` (an int hipStream_t); raise on a non-zero return."""
    l = lib()
    rc = getattr(l, name)(stream, *args)
    if rc != 0:
        msg = l.pdm_last_error().decode("utf-8", "replace")
        raise NativeLibraryError(f"{name} failed with code {rc}: {msg}")


def stream(x):
    """The handle (an int hipStream_t) of the current stream on the device of `x`, a tensor or a device."""
    return torch.cuda.current_stream(getattr(x, "device", x)).cuda_stream


def mfma_a_fragments(w):
    """w (..., Cout, K), both multiples of 16 -> (..., Cout / 16, K / 16, 64, 4), the A fragments of mfma_f32_16x16x4f32
    (csrc/mfma_f32.h): [nb][kb][lane][j] = w[16 nb + (lane & 15)][16 kb + 4 (lane >> 4) + j].  A permutation only, on any device;
    the packers order the block axes as their kernel walks them."""
    lead, (cout, k) = w.shape[:-2], w.shape[-2:]
    assert cout % 16 == 0 and k % 16 == 0, (cout, k)
    n = len(lead)
    w = w.reshape(*lead, cout // 16, 16, k // 16, 4, 4)                  # (nb, i, kb, g, j)
    return w.permute(*range(n), n, n + 2, n + 3, n + 1, n + 4).reshape(*lead, cout // 16, k // 16, 64, 4)


def host_array(ctype, values):
    """A ctypes array of `values`, passed as it is for a pointer parameter and alive for the call; at least one element,
    so that an empty list still gives a valid pointer."""
    if ctype is not ctypes.c_void_p:
        kind = float if ctype in (ctypes.c_float, ctypes.c_double) else int
        values = [kind(v) for v in values]
    return (ctype * max(len(values), 1))(*values)


def check_map(name, t, B, H, W, channels=None):
    """A head's map as an operator takes it: fp32 or bf16 (B, C, H, W) on the GPU with any strides; C = channels when given."""
    assert t.is_cuda and t.dim() == 4 and t.dtype in (torch.float32, torch.bfloat16), f'{name}: fp32 or bf16 (B, C, H, W) on the GPU'
    if channels is None:
        assert t.shape[0] == B and t.shape[2] == H and t.shape[3] == W, f'{name}: {tuple(t.shape)}'
    else:
        assert tuple(t.shape) == (B, channels, H, W), f'{name}: {tuple(t.shape)}, expected {(B, channels, H, W)}'


def map_tables(maps, slots=None):
    """The host tables an entry point takes for a list of maps (csrc/loss_kit.h MapRef): device pointers, bf16 flags and
    4 element strides (b, c, y, x) per entry.  A None entry, and the padding up to `slots` entries, is a null pointer with
    flag 0 and zero strides."""
    maps = list(maps)
    if slots is not None:
        assert len(maps) <= slots, f'{len(maps)} maps for {slots} slots'
        maps += [None] * (slots - len(maps))
    ptrs = host_array(ctypes.c_void_p, [None if t is None else t.data_ptr() for t in maps])
    bf = host_array(ctypes.c_int, [0 if t is None else int(t.dtype == torch.bfloat16) for t in maps])
    st = host_array(ctypes.c_longlong, [s for t in maps for s in ((0, 0, 0, 0) if t is None else t.stride())])
    return ptrs, bf, st


def channel_tables(maps):
    """map_tables' sibling for an entry point that takes every channel of the maps as a (B, H, W) plane of its own, in
    order: the planes' device pointers, bf16 flags and 3 element strides (b, y, x) per plane."""
    ptrs, bf, st = [], [], []
    for t in maps:
        sb, sc, sh, sw = t.stride()
        for c in range(t.shape[1]):
            ptrs.append(t.data_ptr() + c * sc * t.element_size())
            bf.append(int(t.dtype == torch.bfloat16))
            st += [sb, sh, sw]
    return host_array(ctypes.c_void_p, ptrs), host_array(ctypes.c_int, bf), host_array(ctypes.c_longlong, st)


# Cooperating-workgroup FPS calls (n > 16384) whose status word has not been read yet: (workspace, b, n, event).
# The word is read without stalling the caller: when a later call finds the event complete, or in fps_check().
_fps_pending = []


def fps_watch(ws, b, n):
    """Remember a cooperating-workgroup FPS call for a deferred status check (not during graph capture: a captured
    launch is checked by whoever replays the graph, with fps_check_workspace)."""
    if torch.cuda.is_current_stream_capturing():
        return
    fps_check(wait=False)
    ev = torch.cuda.Event()
    ev.record()
    _fps_pending.append((ws, b, n, ev))


def fps_check_workspace(ws, b, n):
    """Synchronise and raise if the cooperating-workgroup FPS that used `ws` gave up waiting for a peer workgroup."""
    flag = ctypes.c_int(0)
    call("pdm_furthest_point_sampling_status", stream(ws), b, n, ws.data_ptr(), ctypes.byref(flag))
    if flag.value:
        raise NativeLibraryError(
            f"furthest_point_sampling ({b} clouds x {n} points): a workgroup gave up waiting for its peers — they were "
            "not co-resident (device shared, partitioned or CU-masked); the sample indices of that call are invalid")


def fps_check(wait=True):
    """Check the status words of earlier cooperating-workgroup FPS calls: all of them (synchronising) or, with
    wait=False, those that have finished."""
    keep = []
    for item in _fps_pending:
        ws, b, n, ev = item
        if wait or ev.query():
            fps_check_workspace(ws, b, n)
        else:
            keep.append(item)
    _fps_pending[:] = keep


def copy_many(dst, src, live=None):
    """dst[k].copy_(src[k]) for lists of same-shaped contiguous CUDA tensors, in one kernel launch.
    live[k] = None | (count, unit): `count` a 1-element int32 CUDA tensor (view) read ON THE DEVICE when the copy runs —
    only the first count * unit bytes of buffer k are live and copied (worst-case-sized buffers, fused.sa_pack)."""
    n = len(dst)
    assert n == len(src)
    if n == 0:
        return
    if live is not None and any(x is not None for x in live):
        assert len(live) == n
        for d, s_ in zip(dst, src):
            assert d.is_contiguous() and s_.is_contiguous() and d.dtype == s_.dtype and d.shape == s_.shape, (d.shape, s_.shape)
        call("pdm_copy_many_dyn", stream(dst[0]), n, host_array(ctypes.c_void_p, [d.data_ptr() for d in dst]),
             host_array(ctypes.c_void_p, [s_.data_ptr() for s_ in src]),
             host_array(ctypes.c_size_t, [d.numel() * d.element_size() for d in dst]),
             host_array(ctypes.c_void_p, [None if x is None else x[0].data_ptr() for x in live]),
             host_array(ctypes.c_uint, [0 if x is None else x[1] for x in live]))
        return
    for d, s_ in zip(dst, src):
        assert d.is_contiguous() and s_.is_contiguous() and d.dtype == s_.dtype and d.shape == s_.shape, (d.shape, s_.shape)
    call("pdm_copy_many", stream(dst[0]), n, host_array(ctypes.c_void_p, [d.data_ptr() for d in dst]),
         host_array(ctypes.c_void_p, [s_.data_ptr() for s_ in src]),
         host_array(ctypes.c_size_t, [d.numel() * d.element_size() for d in dst]))
