"""Guard bands around what the package allocates and what the tests upload.

The operator wrappers of blind_image_denoising_amd allocate their outputs through the name `torch` in their own module.  While
`guards()` (or the `guard_bands` fixture) is active that name is a proxy: everything is forwarded to torch, except that
empty / empty_like / zeros / zeros_like / ones / ones_like / full / full_like (and Tensor.new_empty / new_zeros called from the
package) come from the MIDDLE of a uint8 buffer of GUARD + nbytes + GUARD bytes:

    GUARD = min(max(64 KiB, nbytes rounded up to 4 KiB), 16 MiB)            a multiple of 4096, so data_ptr() % 4096 is what a
                                                                            plain allocation has and kernels pick the same path
    the second guard starts at the tensor's last byte, without rounding     an overrun of one element is seen

Guards hold the word 0x7FC5A5A5 (the sentinel of test_gpu_pair_store.py: a quiet NaN as fp32).  The body of an `empty` tensor
holds the same word as fp32, the half word 0x7FC5 as f16 / bf16 (a NaN in both; the low half of the word would be a finite f16), a
NaN with the word in its low half as fp64, and for integer types a byte chosen by the caller (0x00 or 0xFF, see `twice`).  zeros,
ones and full keep their content and only gain guards.  `dev()` uploads test inputs into such buffers; the guards of an integer
input hold the caller's byte, because a byte has no NaN.

So, with no change to an existing assertion:
  * a store outside an allocation changes a guard: the check at exit names the allocating call site, the side and the byte;
  * a float element that is never written is a NaN in the result (assert_close refuses it, array_equal is False on it);
  * a float load outside an input that reaches the result makes it NaN;
  * an integer element never written, or an integer load outside an input, differs between the two fills: `twice`.

Under the `guard_bands` fixture the test module's own `torch` is the proxy as well, so the outputs a test allocates itself and hands
straight to a C entry point are guarded and sentinel-filled too.

Nothing is intercepted while a stream is capturing (a fill would become part of the graph and a check would synchronise), and the
check runs once, after a torch.cuda.synchronize(), when the context ends."""
import contextlib
import sys
import types

import numpy as np
import pytest
import torch

PACKAGE = "blind_image_denoising_amd"
SENTINEL = 0x7FC5A5A5
SENTINEL16 = 0x7FC5
SENTINEL64 = 0x7FF8A5A57FC5A5A5
PAGE = 4096
MIN_GUARD = 64 << 10
MAX_GUARD = 16 << 20
INT_FILLS = (0x00, 0xFF)

_THIS = __name__
_SESSION = []          # the active session, if any


def guard_bytes(nbytes: int, cap: int = MAX_GUARD) -> int:
    return min(max(MIN_GUARD, -(-nbytes // PAGE) * PAGE), cap)


def _word_of_byte(byte: int) -> int:
    return byte * 0x01010101


def _as_i32(word: int) -> int:
    return word - (1 << 32) if word >= (1 << 31) else word


def _as_i64(word: int) -> int:
    return word - (1 << 64) if word >= (1 << 63) else word


def _call_site():
    """(module, line) of the first frame outside this file"""
    f = sys._getframe(1)
    while f is not None and f.f_globals.get("__name__") == _THIS:
        f = f.f_back
    if f is None:
        return "?", 0
    return f.f_globals.get("__name__", "?"), f.f_lineno


class _Record:
    __slots__ = ("big", "guard", "nbytes", "word", "site", "what")

    def __init__(self, big, guard, nbytes, word, site, what):
        self.big, self.guard, self.nbytes, self.word, self.site, self.what = big, guard, nbytes, word, site, what

    def _pattern(self):
        return torch.tensor(list(int(self.word & 0xFFFFFFFF).to_bytes(4, "little")), dtype=torch.uint8, device=self.big.device)

    def intact(self):
        """0-d bool tensor on the buffer's device: both guards still hold their fill"""
        words = self.big.view(torch.int32)
        w = _as_i32(self.word)
        start = self.guard + self.nbytes
        aligned = -(-start // 4) * 4
        ok = (words[:self.guard // 4] == w).all() & (words[aligned // 4:] == w).all()
        if aligned != start:
            ok = ok & (self.big[start:aligned] == self._pattern()[start % 4:]).all()
        return ok

    def first_damage(self):
        """(side, byte offset) of the changed guard byte at the lowest address.  Before the start the offset counts back from the
        tensor's first byte (-1 is the byte in front of it), after the end it counts from the first byte behind the tensor (0).
        None if both guards are whole."""
        pat = self._pattern()
        for side, lo, hi, origin in (("before the start", 0, self.guard, self.guard),
                                     ("after the end", self.guard + self.nbytes, self.big.numel(), self.guard + self.nbytes)):
            want = pat[torch.arange(lo, hi, device=self.big.device) % 4]
            bad = torch.nonzero(self.big[lo:hi] != want)
            if bad.numel():
                return side, lo + int(bad[0, 0]) - origin
        return None


class _Session:
    def __init__(self, cpu: bool, cap: int):
        self.cpu, self.cap = cpu, cap
        self.int_byte = INT_FILLS[0]
        self.records = []

    # ---- serving ------------------------------------------------------------------------------------------------------------
    def wants(self, device: torch.device) -> bool:
        if device.type == "cpu":
            return self.cpu
        return not torch.cuda.is_current_stream_capturing()

    def serve(self, shape, dtype, device, body, guard_word=SENTINEL, what="empty"):
        """a contiguous tensor of `shape` / `dtype` in the middle of a guarded buffer.  body: None = the unwritten fill of the dtype,
        "keep" = left to the caller, any number = that value."""
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * dtype.itemsize
        guard = guard_bytes(nbytes, self.cap)
        total = -(-(guard + nbytes + guard) // 4) * 4
        big = torch.empty(total, dtype=torch.uint8, device=device)
        big.view(torch.int32).fill_(_as_i32(guard_word))
        t = big[guard:guard + nbytes].view(dtype).view(shape)
        if body is None:
            if dtype == torch.float32:
                if guard_word != SENTINEL:
                    t.view(torch.int32).fill_(_as_i32(SENTINEL))
            elif dtype in (torch.float16, torch.bfloat16):
                t.view(torch.int16).fill_(SENTINEL16)
            elif dtype == torch.float64:
                t.view(torch.int64).fill_(_as_i64(SENTINEL64))
            elif dtype == torch.bool:
                t.fill_(bool(self.int_byte & 1))
            else:
                big[guard:guard + nbytes].fill_(self.int_byte)
        elif body != "keep":
            t.fill_(body)
        self.records.append(_Record(big, guard, nbytes, guard_word, _call_site(), f"{what} {tuple(shape)} {dtype}"))
        return t

    # ---- checking -----------------------------------------------------------------------------------------------------------
    def check(self):
        records, self.records = self.records, []
        if not records:
            return
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        by_device = {}
        for r in records:
            by_device.setdefault(r.big.device, []).append(r.intact())
        if all(bool(torch.stack(oks).all()) for oks in by_device.values()):
            return
        for r in records:
            damage = r.first_damage()
            if damage is not None:
                side, off = damage
                raise AssertionError(f"guard band written: {r.what} allocated at {r.site[0]}:{r.site[1]}, {side}, byte offset {off}")
        raise AssertionError("a guard band was written, but no damaged byte was found on the second look")


def _size_of(args):
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = args[0]
    return tuple(int(s) for s in args)


def _plain(kwargs, allowed=("dtype", "device")):
    """True if the keyword arguments ask for nothing but a dense tensor of a dtype on a device"""
    for k, v in kwargs.items():
        if k in allowed:
            continue
        if k == "requires_grad" and v is False:
            continue
        if k == "pin_memory" and v is False:
            continue
        if k == "layout" and v in (None, torch.strided):
            continue
        if k == "memory_format" and v in (None, torch.contiguous_format):
            continue
        return False
    return True


def _device_of(device):
    if device is None:
        return torch.get_default_device() if hasattr(torch, "get_default_device") else torch.device("cpu")
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


class _TorchProxy(types.ModuleType):
    """stands for the module `torch` in a module of the package: the allocation calls are served from guarded buffers, every other
    attribute (Tensor, the dtypes, cuda, nn, ...) is torch's own"""

    def __init__(self, session):
        super().__init__("torch")
        self.__dict__["_session"] = session

    def __getattr__(self, name):
        return getattr(torch, name)

    def _new(self, real, body, what, args, kwargs, fill_value=None):
        s = self.__dict__["_session"]
        if _SESSION and _SESSION[-1] is s and _plain(kwargs):
            try:
                shape = _size_of(args)
            except (TypeError, ValueError):
                shape = None
            if shape is not None and all(n >= 0 for n in shape):
                dtype = kwargs.get("dtype")
                if dtype is None:
                    dtype = torch.get_default_dtype() if fill_value is None else real((), fill_value).dtype
                device = _device_of(kwargs.get("device"))
                if s.wants(device):
                    return s.serve(shape, dtype, device, body, what=what)
        if fill_value is not None:
            return real(*args, fill_value, **kwargs)
        return real(*args, **kwargs)

    def _like(self, real, body, what, x, kwargs, fill_value=None):
        s = self.__dict__["_session"]
        ok = _SESSION and _SESSION[-1] is s and isinstance(x, torch.Tensor) and x.is_contiguous() and x.layout == torch.strided
        if ok and _plain(kwargs, allowed=("dtype", "device")) and not x.requires_grad:
            device = _device_of(kwargs.get("device")) if kwargs.get("device") is not None else x.device
            if s.wants(device):
                return s.serve(tuple(x.shape), kwargs.get("dtype") or x.dtype, device, body, what=what)
        if fill_value is not None:
            return real(x, fill_value, **kwargs)
        return real(x, **kwargs)

    def empty(self, *size, **kw):
        return self._new(torch.empty, None, "empty", size, kw)

    def zeros(self, *size, **kw):
        return self._new(torch.zeros, 0, "zeros", size, kw)

    def ones(self, *size, **kw):
        return self._new(torch.ones, 1, "ones", size, kw)

    def full(self, size, fill_value, **kw):
        if isinstance(fill_value, torch.Tensor):
            return torch.full(size, fill_value, **kw)
        return self._new(torch.full, fill_value, "full", (size,), kw, fill_value=fill_value)

    def empty_like(self, x, **kw):
        return self._like(torch.empty_like, None, "empty_like", x, kw)

    def zeros_like(self, x, **kw):
        return self._like(torch.zeros_like, 0, "zeros_like", x, kw)

    def ones_like(self, x, **kw):
        return self._like(torch.ones_like, 1, "ones_like", x, kw)

    def full_like(self, x, fill_value, **kw):
        if isinstance(fill_value, torch.Tensor):
            return torch.full_like(x, fill_value, **kw)
        return self._like(torch.full_like, fill_value, "full_like", x, kw, fill_value=fill_value)


def _tensor_method(session, name, body):
    """Tensor.new_empty / new_zeros: guarded when the caller is a module of the package, torch's own otherwise"""
    real = getattr(torch.Tensor, name)

    def method(self, *size, **kw):
        caller = sys._getframe(1).f_globals.get("__name__", "")
        if _SESSION and _SESSION[-1] is session and (caller == PACKAGE or caller.startswith(PACKAGE + ".")) and _plain(kw):
            try:
                shape = _size_of(size)
            except (TypeError, ValueError):
                return real(self, *size, **kw)
            device = _device_of(kw.get("device")) if kw.get("device") is not None else self.device
            if session.wants(device) and self.layout == torch.strided:
                return session.serve(shape, kw.get("dtype") or self.dtype, device, body, what=name)
        return real(self, *size, **kw)

    return method


def _native_scratch(session, native):
    """_native.scratch imports torch inside the function, out of the proxy's reach: the fp64 scratch tensor it sized is replaced by
    a guarded one of the same shape, filled as an `empty` one"""
    real = native.scratch

    def scratch(entry, device, *dims):
        t, nbytes = real(entry, device, *dims)
        if _SESSION and _SESSION[-1] is session and session.wants(t.device):
            t = session.serve(tuple(t.shape), t.dtype, t.device, None, what="scratch")
        return t, nbytes

    return real, scratch


@contextlib.contextmanager
def guards(cpu: bool = False, cap: int = MAX_GUARD, also=()):
    """Interpose on every module of the package that is loaded when the context starts (one imported for the first time inside it
    keeps torch itself until the next context; the package's __init__ imports them all), and on the modules in `also` -- the
    test module, whose own outputs for direct C entry calls then lie between guards too.  All guards are checked at exit.  Inside
    an active context it is that context."""
    if _SESSION:
        yield _SESSION[-1]
        return
    session = _Session(cpu, cap)
    proxy = _TorchProxy(session)
    patched = []
    saved = {}
    try:
        for name, mod in list(sys.modules.items()):
            if mod is not None and (name == PACKAGE or name.startswith(PACKAGE + ".")) and mod.__dict__.get("torch") is torch:
                mod.torch = proxy
                patched.append(mod)
        for mod in also:
            if mod.__dict__.get("torch") is torch:
                mod.torch = proxy
                patched.append(mod)
        for name, body in (("new_empty", None), ("new_zeros", 0)):
            saved[name] = torch.Tensor.__dict__.get(name)
            setattr(torch.Tensor, name, _tensor_method(session, name, body))
        native = sys.modules.get(PACKAGE + "._native")
        if native is not None:
            saved["scratch"], native.scratch = _native_scratch(session, native)
        _SESSION.append(session)
        yield session
    except BaseException:
        session.records = []          # the body's own error is the news
        raise
    finally:
        if _SESSION and _SESSION[-1] is session:
            _SESSION.pop()
        if "scratch" in saved:
            native.scratch = saved.pop("scratch")
        for name, old in saved.items():
            if old is None:
                delattr(torch.Tensor, name)
            else:
                setattr(torch.Tensor, name, old)
        for mod in patched:
            mod.torch = torch
    session.check()


@pytest.fixture
def guard_bands(request):
    """the test body runs under guards(), the test module's own `torch` included: what a test allocates on the device for a direct
    call of a C entry point is guarded like what a wrapper allocates.  The teardown synchronises and checks every guard."""
    with guards(also=(request.module,)) as session:
        yield session


# ---- test inputs ---------------------------------------------------------------------------------------------------------------

def dev(a, dtype=None, device="cuda"):
    """upload `a` (anything np.asarray takes, or a CPU tensor; None stays None).  Under guards the copy lies between guard bands: the
    NaN word around floats, the session's integer byte around integers."""
    if a is None:
        return None
    host = a.detach().contiguous() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))
    if not _SESSION:
        return host.to(device)
    s = _SESSION[-1]
    word = SENTINEL if host.dtype.is_floating_point else _word_of_byte(s.int_byte)
    t = s.serve(tuple(host.shape), host.dtype, _device_of(device), "keep", guard_word=word, what="input")
    t.copy_(host)
    return t


def dev_f32(a, dtype=np.float32):
    """helpers.dev with guards: float32 unless another dtype is named"""
    return dev(a, dtype)


# ---- what was left unwritten ---------------------------------------------------------------------------------------------------

def unwritten(t: torch.Tensor) -> int:
    """the number of elements of a float tensor that still hold the fill of a guarded torch.empty"""
    t = t.contiguous()
    if t.dtype == torch.float32:
        return int((t.view(torch.int32) == _as_i32(SENTINEL)).sum())
    if t.dtype in (torch.float16, torch.bfloat16):
        return int((t.view(torch.int16) == SENTINEL16).sum())
    if t.dtype == torch.float64:
        return int((t.view(torch.int64) == _as_i64(SENTINEL64)).sum())
    raise TypeError(f"unwritten() is for float tensors, got {t.dtype}: run integer outputs through twice()")


def _bits(x):
    """the result of an operator as nested tuples of (dtype, shape, bytes)"""
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            torch.cuda.synchronize()
        x = x.detach().cpu().contiguous()
        return (str(x.dtype), tuple(x.shape), x.view(torch.uint8).numpy().tobytes() if x.numel() else b"")
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, dict):
        return tuple((k, _bits(v)) for k, v in sorted(x.items()))
    if isinstance(x, (tuple, list)):
        return tuple(_bits(v) for v in x)
    return x


def _first_difference(a, b, path="result"):
    if isinstance(a, tuple) and len(a) == 3 and isinstance(a[2], bytes):
        if a[:2] != b[:2]:
            return f"{path}: {a[:2]} against {b[:2]}"
        if a[2] != b[2]:
            d = np.nonzero(np.frombuffer(a[2], np.uint8) != np.frombuffer(b[2], np.uint8))[0]
            return f"{path} {a[0]} {a[1]}: {d.size} bytes differ, the first at byte offset {int(d[0])}"
        return None
    if isinstance(a, tuple) and isinstance(b, tuple) and len(a) == len(b):
        for i, (u, v) in enumerate(zip(a, b)):
            msg = _first_difference(u, v, f"{path}[{i}]")
            if msg:
                return msg
        return None
    return None if a == b else f"{path}: {a!r} against {b!r}"


def twice(fn, cpu: bool = False):
    """fn() under both integer fills (the bodies of integer `empty` tensors and the guards around integer inputs hold 0x00, then
    0xFF; inputs must be uploaded with dev() inside fn).  The two results must be bit-identical: an integer element that nothing
    writes, or an integer load outside an input, is not.  Returns the first result."""
    with guards(cpu=cpu) as s:
        results = []
        before = s.int_byte
        try:
            for byte in INT_FILLS:
                s.int_byte = byte
                results.append(fn())
        finally:
            s.int_byte = before
        diff = _first_difference(_bits(results[0]), _bits(results[1]))
        assert diff is None, f"the result depends on the fill of unwritten integer memory (0x00 against 0xFF): {diff}"
        return results[0]
