"""ctypes binding of libepn_so3conv.so on torch device tensors, derived from include/epn_so3conv.h.

PyTorch is plumbing here: it owns device memory and the current HIP stream; every compute call goes
through the C ABI.  There is NO CPU or eager fallback: a missing library or a non-device tensor
raises (the reference's extensions do the same through CHECK_CUDA, grouping_cuda.cpp:66-68).

The header is the one copy of every signature: the compiler holds the .hip files to it, and parse_header() reads this
binding's argument and return types, its export list and its struct layouts from it.  A new entry point is added to the
header and nowhere else.
"""
import ctypes
import os
import re

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EPN_LIB", os.path.join(_PKG, "libepn_so3conv.so"))   # EPN_LIB: A/B builds (tools/)
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "epn_so3conv.h")   # the file build.py compiles against

ABI_VERSION = 3          # the EPN_ABI_VERSION this package's callers were written against

# C type -> ctypes type, for parameters and struct fields and for return values.  On top of the first table any pointer
# (`const float *const *` included) is a c_void_p, and a pointer to one of the header's structs a POINTER(its Structure).
# A type that stands in neither fails the load: a new one in the header is added here, never guessed.
_ARG_TYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
              "long long": ctypes.c_longlong, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
              "epn_stream_t": ctypes.c_void_p}
_RETURN_TYPES = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong,
                 "const char *": ctypes.c_char_p}
_DECLARATOR = re.compile(r"([^,]*[\s*])?(\w+)\s*(?:,|$)")        # `const void *A, *Bt` -> (`const void *`, `A`), (`*`, `Bt`)


def parse_header(path):
    """(signatures, structs, host_only) of a header written like include/epn_so3conv.h: {name: (restype, (argtypes))} of
    every `ret epn_name(params);` in header order, {C name: Structure class} of every `typedef struct epn_x {...} epn_x;`,
    and the set of names declared without an epn_stream_t parameter."""
    try:
        with open(path) as f:
            src = f.read()
    except OSError as e:
        raise RuntimeError(f"{path} cannot be read ({e.strerror}): the binding takes every signature from the C header, "
                           "which belongs at <package>/../include/epn_so3conv.h. epn_pointcloud_amd keeps no second copy.")
    src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", src, flags=re.S)
    src = re.sub(r"^[ \t]*#.*$", "", src, flags=re.M)

    def spell(c):
        return " ".join(c.replace("*", " * ").split())         # one spelling per type: `const char *`

    def declared(text, where, shared_type=False):
        """`const void *A, *Bt` -> [(`const void *`, `A`), (`const void *`, `Bt`)]; only struct fields may share a type"""
        found, out, base = _DECLARATOR.findall(text), [], ""
        for c, name in found:
            own = c.rstrip("* \t\n")
            base = own or (shared_type and base)
            if not base:
                break                                          # a name without a type, such as an unnamed parameter
            out.append((spell(f"{base} {c[len(own):]}"), name))
        if len(out) != text.count(",") + 1:
            raise RuntimeError(f"{path}: {where}: cannot read the declaration `{spell(text)}`")
        return out

    def ctype(c, where, table):
        if c in table:
            return table[c]
        if table is _ARG_TYPES and c.endswith("*"):
            pointee = structs.get(c.replace("const ", "")[:-2])
            return ctypes.POINTER(pointee) if pointee else ctypes.c_void_p
        raise RuntimeError(f"{path}: {where} has the C type `{c}`, which the binding has no ctypes type for "
                           f"(it knows {', '.join(table)}{' and pointers' if table is _ARG_TYPES else ''})")

    structs = {}
    for name, body in re.findall(r"typedef\s+struct\s+(epn_\w+)\s*\{(.*?)\}\s*\1\s*;", src, flags=re.S):
        fields = [(f, ctype(c, f"field `{f}` of struct {name}", _ARG_TYPES))
                  for d in body.split(";") if d.strip() for c, f in declared(d, f"struct {name}", shared_type=True)]
        structs[name] = type("".join(w.capitalize() for w in name[4:].split("_")), (ctypes.Structure,),
                             {"_fields_": fields, "__doc__": f"struct {name} ({os.path.basename(path)})."})

    signatures, host_only = {}, set()
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(epn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        params = [] if params.strip() == "void" else declared(params, name)
        signatures[name] = (ctype(spell(ret), f"the return value of {name}", _RETURN_TYPES),
                            tuple(ctype(c, f"parameter `{p}` of {name}", _ARG_TYPES) for c, p in params))
        if all(c != "epn_stream_t" for c, _ in params):
            host_only.add(name)
    return signatures, structs, host_only


# Read when the module is imported: EXPORTS and the struct classes are module attributes that callers use before get_lib().
_SIGNATURES, _STRUCTS, _HOST_ONLY = parse_header(HEADER_PATH)
EXPORTS = list(_SIGNATURES)          # header order; _HOST_ONLY: no stream argument, nothing launched, handed out unwrapped
InterDesc, NormPairSide, NormPairFrozenSide, GemmNtProblem, GemmTnProblem = (
    _STRUCTS["epn_" + n] for n in ("inter_desc", "norm_pair_side", "norm_pair_frozen_side", "gemm_nt_problem", "gemm_tn_problem"))


def signatures():
    """{name: (restype, (argtypes))} of every entry point the header declares, in its order; the library is not loaded."""
    return dict(_SIGNATURES)


_lib = None


def get_lib():
    """Load the HIP library or fail loudly (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension was not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
            "epn_pointcloud_amd has no CPU/eager fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    try:
        got = int(lib.epn_abi_version())
    except AttributeError:
        got = None
    if got != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} implements ABI revision {got}, this binding expects {ABI_VERSION} "
                           "(include/epn_so3conv.h EPN_ABI_VERSION): rebuild the library -- signatures differ between revisions")
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype, fn.argtypes = restype, list(argtypes)
    _lib = _LibProxy(lib)
    return _lib


CALL_HOOK = None      # ops.profile_begin(): callable(name, fn, args) -> rc, brackets every launching call with HIP events


class _StreamArg(ctypes.c_void_p):
    """epn_stream_t argument that remembers its device, and the device to switch back to after the call (stream_of)."""
    restore = None
    device = None


class _LibProxy:
    """The CDLL with every launching entry point wrapped: (i) the current device, if stream_of() had to switch it to the
    tensors' device for the launch, is restored afterwards -- a scoped guard like ATen's, not a permanent set_device;
    (ii) an optional hook (CALL_HOOK) sees every call, so a benchmark can time ALL of them, not only the ones a
    caller chose to bracket."""

    def __init__(self, lib):
        object.__setattr__(self, "_cdll", lib)

    def __getattr__(self, name):
        fn = getattr(self._cdll, name)
        if name in _HOST_ONLY:
            object.__setattr__(self, name, fn)
            return fn

        def call(*args):
            hook = CALL_HOOK
            st = args[-1] if args else None
            prev = getattr(st, "restore", None)
            dev = getattr(st, "device", None)
            if dev is not None and torch.cuda.current_device() != dev:
                # a stream argument used for a SECOND call (stream_of()'s switch was undone when the first returned): the
                # proxy makes the stream's device current itself and restores whatever was current
                prev = torch.cuda.current_device() if prev is None else prev
                torch.cuda.set_device(dev)
            try:
                return fn(*args) if hook is None else hook(name, fn, args)
            finally:
                if prev is not None:
                    torch.cuda.set_device(prev)
        call.__name__ = name
        object.__setattr__(self, name, call)
        return call


class kernel_policy:
    """`with _lib.kernel_policy(n):` -- epn_set_kernel_policy(n) for the block (1 = generic kernels, 2 = the first layer's VALU
    kernel instead of its matrix-pipe form); cross-checks only."""

    def __init__(self, policy):
        self.policy = int(policy)

    def __enter__(self):
        check(get_lib().epn_set_kernel_policy(self.policy), "set_kernel_policy")

    def __exit__(self, *exc):
        check(get_lib().epn_set_kernel_policy(0), "set_kernel_policy")


def generic_kernels():
    """`with _lib.generic_kernels():` -- run on the any-shape generic kernels (cross-check tests only)."""
    return kernel_policy(1)


def check(rc, what):
    if rc != 0:
        msg = get_lib().epn_strerror(int(rc)).decode()
        raise RuntimeError(f"{what} failed: {msg} (code {rc})")


def stream_of(t):
    """Current torch stream of t's device, as the epn_stream_t argument of the call being made.  The HIP runtime launches
    on ITS current device, so that is switched to t's device first when it differs (a tensor on cuda:1 while cuda:0 is
    current must not launch on cuda:0); the returned argument carries the device to switch back to, and the library
    proxy restores it when the call returns -- the scoped guard the reference's extensions get from ATen."""
    dev = t.device
    arg = _StreamArg(torch.cuda.current_stream(dev).cuda_stream)
    arg.device = dev.index
    if dev.index is not None and torch.cuda.current_device() != dev.index:
        arg.restore = torch.cuda.current_device()
        torch.cuda.set_device(dev)
    return arg


def same_device(*tensors):
    """All device tensors of one call must live on one device (checked where several tensors meet)."""
    devs = {t.device for t in tensors if t is not None}
    if len(devs) > 1:
        raise RuntimeError(f"tensors of one call are on different devices: {sorted(str(d) for d in devs)}")


def float_dtype(t, name):
    """float32 or float64: the dtypes the reference's index / gather extensions dispatch on."""
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{name} must be float32 or float64, got {t.dtype}")
    return t.dtype


def dev_ptr(t, name, dtype=torch.float32):
    """Pointer of a device tensor; mirrors the reference's CHECK_INPUT (grouping_cuda.cpp:66-68)."""
    if t is None:
        return ctypes.c_void_p(0)
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")  # ROCm devices are 'cuda' in torch
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return ctypes.c_void_p(t.data_ptr())
