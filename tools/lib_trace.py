"""The call trace the digest tools hash (tape_digest.py, backbone_tape_digest.py, click_round_digest.py, engine_digest.py):
every symbol of the loaded library is wrapped so that each call appends ``(symbol, every argument passed by value)`` to one
list -- pointers (c_void_p, POINTER(...)) differ from run to run and are left out.  Only ``lib.load()``, ``lib.SYMBOLS`` and
setattr on the loaded library are used, so the tools run on any commit that has those (to compare with an older commit, copy
the tool and this file into its ``tools/``)."""
import ctypes
import hashlib


def plain(a):
    """A by-value argument as something with a stable repr: numbers as they are, a struct as the tuple of its fields."""
    if isinstance(a, ctypes.Structure):
        return tuple(plain(getattr(a, f[0])) for f in a._fields_)
    return getattr(a, "value", a)


def install(convert=plain):
    """Wrap the library's symbols; returns the list the calls are appended to (``del trace[:]`` starts a new section)."""
    from agile3d_amd import lib as L
    lib, trace = L.load(), []
    for name, (_, argtypes) in L.SYMBOLS.items():
        by_value = [i for i, t in enumerate(argtypes) if t is not ctypes.c_void_p and not hasattr(t, "contents")]
        fn = getattr(lib, name)
        setattr(lib, name, lambda *a, _fn=fn, _n=name, _v=by_value: (trace.append((_n,) + tuple(convert(a[i]) for i in _v)), _fn(*a))[1])
    return trace


def digest(trace):
    return hashlib.sha256(repr(trace).encode()).hexdigest()
