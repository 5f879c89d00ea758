"""A numpy stand-in for the ``jax`` names the reference's sampling controller uses.

TEST INFRASTRUCTURE ONLY.  ``oracle/record_srbd_reference.py`` installs these modules into ``sys.modules`` and then
executes the reference's files from a checkout, unmodified; ``tests/test_jax_standin.py`` checks the stand-in's own
semantics against plain numpy.  The product path never imports this module.

It is written from JAX's public semantics (x64 off), not from any reference text:

* arrays are an ``ndarray`` subclass (``Array``) with the functional ``.at[idx].set(v)`` (a copy is returned), 0-d
  results instead of numpy scalars, and ``+=`` and friends rebinding instead of writing in place;
* dtypes: Python floats and float lists become float32, ``arange`` and integer lists int32, ``linspace`` float32; a
  Python scalar is weak (it takes the array operand's type; a Python float against an integer array gives the default
  float); no float64 or int64 value survives an operation;
* ``set_default_float(numpy.float64)`` switches the default float (JAX with x64 on): float32 arrays stay float32 and
  promote against float64 as numpy does.  The recorder uses it for its conditioning check only;
* ``jit`` returns the function (``device=`` ignored), ``vmap`` is a Python loop over axis 0 of the mapped arguments,
  ``lax.fori_loop`` is a Python loop with an int32 index, ``devices()`` is one dummy object, ``config.update`` does
  nothing;
* ``jax.random`` is ``oracle/jax_random_oracle.py`` (bit-exact to the published threefry stream,
  ``tests/test_jax_random.py``); the draws are float32 and are cast up in the float64 mode;
* ``cov`` follows JAX's published algorithm in the working precision (centre, ``X @ X.T / (n - 1)``), ``argsort`` is
  stable, ``nanargmin`` returns the first index on ties, an out-of-range index raises (JAX would clamp; the recorder
  must not record a clamped read silently).

What this does not reproduce is XLA's own rounding and reduction order (fused multiply-adds, tree reductions, its
``sin`` / ``cos`` / ``exp``): numpy's IEEE float32 evaluation stands in for them.

Any name missing here raises ``AttributeError`` (plain module attribute lookup): the recorder fails, it does not guess.
"""
from __future__ import annotations

import sys
import types

import numpy as np

from . import jax_random_oracle as _jro

assert int(np.__version__.split(".")[0]) >= 2, "the stand-in relies on numpy 2 (NEP 50) weak Python scalars"

_default_float = np.dtype(np.float32)


def set_default_float(dtype):
    """float32 (x64 off, the reference's setting) or float64 (the recorder's conditioning run)."""
    global _default_float
    dtype = np.dtype(dtype)
    assert dtype in (np.dtype(np.float32), np.dtype(np.float64))
    _default_float = dtype


def default_float():
    return _default_float


def _x64():
    return _default_float == np.dtype(np.float64)


def _canon_dtype(dt):
    dt = np.dtype(dt)
    if not _x64():
        if dt == np.float64:
            return np.dtype(np.float32)
        if dt == np.int64:
            return np.dtype(np.int32)
        if dt == np.uint64:
            return np.dtype(np.uint32)
    return dt


def _is_py_scalar(x):
    return isinstance(x, (bool, int, float)) and not isinstance(x, np.generic)


def _base(x):
    """An operand as numpy sees it: Python scalars untouched (weak), everything else a canonical base ndarray."""
    if _is_py_scalar(x):
        return x
    a = np.asarray(x)
    if isinstance(a, Array):
        a = a.view(np.ndarray)
    dt = _canon_dtype(a.dtype)
    return a if dt == a.dtype else a.astype(dt)


def _wrap(x):
    """A result as an Array of canonical dtype (tuples element by element)."""
    if isinstance(x, tuple):
        return tuple(_wrap(v) for v in x)
    a = np.asarray(x)
    dt = _canon_dtype(a.dtype)
    if dt != a.dtype:
        a = a.astype(dt)
    return a.view(Array)


def _operand_dtype(*xs):
    """The result dtype of mixing ``xs`` under weak Python scalars."""
    strong = [_canon_dtype(np.asarray(x).dtype) for x in xs if not _is_py_scalar(x)]
    has_float = any(isinstance(x, float) for x in xs if _is_py_scalar(x))
    if not strong:
        if has_float:
            return _default_float
        return np.dtype(np.bool_) if all(isinstance(x, bool) for x in xs) else np.dtype(np.int32)
    dt = _canon_dtype(np.result_type(*strong))
    if has_float and dt.kind in "biu":
        return _default_float
    if dt.kind == "b" and any(not isinstance(x, bool) for x in xs if _is_py_scalar(x)):
        return np.dtype(np.int32)
    return dt


class _AtIndex:
    def __init__(self, arr, idx):
        self._arr, self._idx = arr, idx

    def set(self, value):
        out = np.array(self._arr.view(np.ndarray), copy=True)
        out[self._idx] = np.asarray(value).astype(out.dtype)
        return out.view(Array)


class _At:
    def __init__(self, arr):
        self._arr = arr

    def __getitem__(self, idx):
        return _AtIndex(self._arr, idx)


class Array(np.ndarray):
    __array_priority__ = 100.0

    def __array_ufunc__(self, ufunc, method, *inputs, out=None, **kwargs):
        if out is not None:
            raise TypeError("the stand-in's arrays are immutable: no out=")
        res = getattr(ufunc, method)(*[_base(x) for x in inputs], **kwargs)
        return _wrap(res)

    def __array_function__(self, func, types_, args, kwargs):
        def strip(v):
            if isinstance(v, Array):
                return v.view(np.ndarray)
            if isinstance(v, (list, tuple)):
                return type(v)(strip(e) for e in v)
            return v

        res = func(*strip(args), **{k: strip(v) for k, v in kwargs.items()})
        if isinstance(res, np.ndarray):
            return res.view(Array)  # numpy called on our arrays keeps numpy's dtypes
        if isinstance(res, (list, tuple)):
            return type(res)(r.view(Array) if isinstance(r, np.ndarray) else r for r in res)
        return res

    def __getitem__(self, idx):
        if isinstance(idx, Array):
            idx = idx.view(np.ndarray)
        elif isinstance(idx, tuple):
            idx = tuple(i.view(np.ndarray) if isinstance(i, Array) else i for i in idx)
        r = np.ndarray.__getitem__(self.view(np.ndarray), idx)
        return np.asarray(r).view(Array)

    def __setitem__(self, idx, value):
        raise TypeError("the stand-in's arrays are immutable: use .at[idx].set(value)")

    def __iter__(self):
        if self.ndim == 0:
            raise TypeError("iteration over a 0-d array")
        return (self[i] for i in range(self.shape[0]))

    @property
    def at(self):
        return _At(self)

    def take(self, index, axis=None):
        return _wrap(np.take(self.view(np.ndarray), np.asarray(index), axis=axis))

    # JAX arrays are immutable: an augmented assignment rebinds the name
    def __iadd__(self, other):
        return self + other

    def __isub__(self, other):
        return self - other

    def __imul__(self, other):
        return self * other

    def __itruediv__(self, other):
        return self / other

    def __matmul__(self, other):
        return _wrap(np.matmul(_base(self), _base(other)))

    def __rmatmul__(self, other):
        return _wrap(np.matmul(_base(other), _base(self)))

    def __imatmul__(self, other):
        return self @ other


# --------------------------------------------------------------------------------------------------------------------
# jax.numpy
# --------------------------------------------------------------------------------------------------------------------
def _array(obj, dtype=None):
    if _is_py_scalar(obj):
        a = np.asarray(obj, dtype=_operand_dtype(obj))
    else:
        a = np.array(_strip_nested(obj))
    if dtype is not None:
        return a.astype(np.dtype(dtype)).view(Array)
    return _wrap(a)


def _strip_nested(obj):
    if isinstance(obj, Array):
        return obj.view(np.ndarray)
    if isinstance(obj, (list, tuple)):
        return [_strip_nested(o) for o in obj]
    return obj


def _shape_dtype(dtype):
    return _default_float if dtype is None else np.dtype(dtype)


def _float_in(x):
    """The operand of a float-valued function: integers and Python scalars become the default float."""
    a = np.asarray(_base(x))
    if _is_py_scalar(x) or a.dtype.kind in "biu":
        return a.astype(_default_float)
    return a


def _unary_float(fn):
    def f(x):
        return _wrap(fn(_float_in(x)))

    f.__name__ = fn.__name__
    return f


def _where(cond, x, y):
    dt = _operand_dtype(x, y)
    return _wrap(np.where(np.asarray(_base(cond)), np.asarray(_base(x)).astype(dt), np.asarray(_base(y)).astype(dt)))


def _scalar_type(np_type):
    def f(x=0):
        return np.asarray(_base(x)).astype(np_type).view(Array)

    f.__name__ = np_type.__name__
    f.dtype = np.dtype(np_type)
    return f


def _tile(a, reps):
    return _wrap(np.tile(np.asarray(_array(a)), reps))


def _concatenate(arrays, axis=0):
    arrays = [_base(a) for a in arrays]
    dt = _operand_dtype(*arrays)
    return _wrap(np.concatenate([np.asarray(a).astype(dt) for a in arrays], axis=axis))


def _split(a, sections, axis=0):
    return [_wrap(p) for p in np.split(_base(a), sections, axis=axis)]


def _dot(a, b):
    a, b = _base(a), _base(b)
    dt = _operand_dtype(a, b)
    return _wrap(np.dot(np.asarray(a).astype(dt), np.asarray(b).astype(dt)))


def _sum(a, axis=None):
    return _wrap(np.sum(_base(a), axis=axis))


def _max(a, axis=None):
    return _wrap(np.max(_base(a), axis=axis))


def _nanargmin(a, axis=None):
    return _wrap(np.asarray(np.nanargmin(_base(a), axis=axis)).astype(np.int32))


def _argsort(a, axis=-1):
    return _wrap(np.argsort(_base(a), axis=axis, kind="stable").astype(np.int32))


def _cov(m, y=None, rowvar=True, bias=False, ddof=None):
    if y is not None:
        raise NotImplementedError("cov(m, y)")
    X = np.atleast_2d(_float_in(m))
    if not rowvar and X.shape[0] != 1:
        X = X.T
    dt = X.dtype
    if ddof is None:
        ddof = 0 if bias else 1
    n = X.shape[1]
    avg = (np.sum(X, axis=1) / dt.type(n)).astype(dt)
    X = (X - avg[:, None]).astype(dt)
    c = (np.dot(X, X.T) / dt.type(n - ddof)).astype(dt)
    return _wrap(c.squeeze() if c.shape == (1, 1) else c)


def _make_numpy_module():
    m = types.ModuleType("jax.numpy")
    m.ndarray = Array
    m.newaxis = None
    m.pi = np.pi
    m.array = _array
    m.asarray = _array
    m.zeros = lambda shape, dtype=None: np.zeros(shape, _shape_dtype(dtype)).view(Array)
    m.ones = lambda shape, dtype=None: np.ones(shape, _shape_dtype(dtype)).view(Array)
    m.identity = lambda n, dtype=None: np.identity(n, _shape_dtype(dtype)).view(Array)
    m.eye = lambda n, dtype=None: np.identity(n, _shape_dtype(dtype)).view(Array)

    def arange(*a, dtype=None):
        r = np.arange(*a)
        if dtype is not None:
            return r.astype(np.dtype(dtype)).view(Array)
        return _wrap(r.astype(_default_float) if r.dtype.kind == "f" else r)

    m.arange = arange
    m.linspace = lambda start, stop, num=50, dtype=None: np.linspace(start, stop, num).astype(
        _shape_dtype(dtype)).view(Array)
    m.tile = _tile
    m.concatenate = _concatenate
    m.split = _split
    m.dot = _dot
    m.sum = _sum
    m.max = _max
    m.where = _where
    m.isnan = lambda x: _wrap(np.isnan(_base(x)))
    m.isinf = lambda x: _wrap(np.isinf(_base(x)))
    m.nanargmin = _nanargmin
    m.argsort = _argsort
    m.cov = _cov
    m.diag = lambda a: _wrap(np.diag(_base(a)))
    for fn in (np.exp, np.sin, np.cos, np.sqrt):
        setattr(m, fn.__name__, _unary_float(fn))
    m.float32 = _scalar_type(np.float32)
    m.float64 = _scalar_type(np.float64)
    m.int16 = _scalar_type(np.int16)
    m.int32 = _scalar_type(np.int32)
    return m


# --------------------------------------------------------------------------------------------------------------------
# jax.random
# --------------------------------------------------------------------------------------------------------------------
def _key_of(key):
    return np.asarray(key).view(np.ndarray).astype(np.uint32).reshape(2)


def _float_draw(a, dtype):
    return np.asarray(a).astype(_shape_dtype(dtype)).view(Array)


def _make_random_module():
    m = types.ModuleType("jax.random")
    m.PRNGKey = lambda seed: _jro.prng_key(seed).view(Array)
    m.key = m.PRNGKey
    m.split = lambda key, num=2: _jro.split(_key_of(key), int(num)).view(Array)
    m.normal = lambda key, shape=(), dtype=None: _float_draw(_jro.normal(_key_of(key), tuple(shape)), dtype)
    m.uniform = lambda key, shape=(), dtype=None, minval=0.0, maxval=1.0: _float_draw(
        _jro.uniform(_key_of(key), tuple(shape), minval, maxval), dtype)

    def randint(key, shape, minval, maxval, dtype=None):
        shape = tuple(shape)
        return _jro.randint(_key_of(key), int(np.prod(shape)), int(minval), int(maxval)).reshape(shape).view(Array)

    def choice(key, a, shape=(), replace=True, p=None):
        if not replace or p is not None:
            raise NotImplementedError("choice without replacement or with p")
        a = np.asarray(_base(_array(a)))
        shape = tuple(shape)
        return _wrap(_jro.choice(_key_of(key), a, int(np.prod(shape))).reshape(shape + a.shape[1:]))

    m.randint = randint
    m.choice = choice
    return m


# --------------------------------------------------------------------------------------------------------------------
# jax, jax.lax
# --------------------------------------------------------------------------------------------------------------------
class _Device:
    platform = "cpu"

    def __repr__(self):
        return "StandInDevice(cpu)"


def _jit(fun=None, **kwargs):
    if fun is None:
        return lambda f: f
    return fun


def _vmap(fun, in_axes=0, out_axes=0):
    if out_axes != 0:
        raise NotImplementedError("vmap: out_axes other than 0")

    def mapped(*args):
        axes = (in_axes,) * len(args) if isinstance(in_axes, int) or in_axes is None else tuple(in_axes)
        if len(axes) != len(args):
            raise ValueError("vmap: in_axes does not match the arguments")
        if any(a not in (None, 0) for a in axes):
            raise NotImplementedError("vmap: mapped axis other than 0")
        sizes = {np.shape(a)[0] for a, ax in zip(args, axes) if ax == 0}
        if len(sizes) != 1:
            raise ValueError("vmap: mapped arguments disagree on the axis size")
        n = sizes.pop()
        outs = [fun(*[(_array(a)[i] if ax == 0 else a) for a, ax in zip(args, axes)]) for i in range(n)]
        if isinstance(outs[0], tuple):
            return tuple(_wrap(np.stack([_base(o[k]) for o in outs])) for k in range(len(outs[0])))
        return _wrap(np.stack([_base(o) for o in outs]))

    return mapped


def _fori_loop(lower, upper, body_fun, init_val):
    val = init_val
    for i in range(int(lower), int(upper)):
        val = body_fun(np.asarray(i, dtype=np.int32).view(Array), val)
    return val


def make_modules():
    """Fresh ``{"jax": ..., "jax.numpy": ..., "jax.random": ..., "jax.lax": ...}`` modules."""
    jax = types.ModuleType("jax")
    jax.__path__ = []
    jnp = _make_numpy_module()
    random = _make_random_module()
    lax = types.ModuleType("jax.lax")
    lax.fori_loop = _fori_loop
    config = types.SimpleNamespace(update=lambda *a, **k: None)
    jax.numpy, jax.random, jax.lax, jax.config = jnp, random, lax, config
    jax.jit, jax.vmap = _jit, _vmap
    jax.devices = lambda backend=None: [_Device()]
    jax.Array = Array
    return {"jax": jax, "jax.numpy": jnp, "jax.random": random, "jax.lax": lax}


def install():
    """Put the stand-in into ``sys.modules`` (the recorder's process only) and return the modules."""
    mods = make_modules()
    sys.modules.update(mods)
    return mods
