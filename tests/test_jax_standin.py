"""oracle/jax_standin.py: the stand-in's own semantics against plain numpy (no reference, no GPU)."""
import numpy as np
import pytest

from oracle import jax_random_oracle as jro
from oracle import jax_standin as js

f32 = np.float32


@pytest.fixture()
def mods():
    js.set_default_float(np.float32)
    yield js.make_modules()
    js.set_default_float(np.float32)


def test_at_set_does_not_alias(mods):
    jnp = mods["jax.numpy"]
    a = jnp.zeros(4)
    b = a.at[1].set(2.5)
    c = b.at[1:3].set(jnp.array([7, 8]))
    np.testing.assert_array_equal(np.asarray(a), [0, 0, 0, 0])
    np.testing.assert_array_equal(np.asarray(b), [0, 2.5, 0, 0])
    np.testing.assert_array_equal(np.asarray(c), [0, 7, 8, 0])
    assert c.dtype == np.float32
    n = jnp.array([-1, -1]).at[0].set(jnp.float32(3.0))
    assert n.dtype == np.int32 and n.tolist() == [3, -1]
    with pytest.raises(TypeError):
        a[0] = 1.0
    d = a
    d += 1.0                      # rebinding, as with an immutable array
    assert np.asarray(a).tolist() == [0, 0, 0, 0] and np.asarray(d).tolist() == [1, 1, 1, 1]


def test_dtype_rules(mods):
    jnp = mods["jax.numpy"]
    assert jnp.array(0.1).dtype == np.float32 and jnp.array([0.5, 1.5]).dtype == np.float32
    assert jnp.array(3).dtype == np.int32 and jnp.array([1, 2]).dtype == np.int32
    assert jnp.arange(5).dtype == np.int32 and jnp.linspace(0, 12, 3).dtype == np.float32
    assert jnp.zeros(3).dtype == np.float32 and jnp.array(np.zeros(3)).dtype == np.float32
    x = jnp.array([1.0, 2.0])
    assert (x * 0.1).dtype == np.float32 and (0.1 / x).dtype == np.float32 and (x + np.eye(2)).dtype == np.float32
    assert float((x * 0.1)[0]) == float(f32(1.0) * f32(0.1))       # the scalar is rounded to float32 first
    i = jnp.array([-1, 3])[1]
    assert i.shape == () and i.dtype == np.int32
    q = i / 6.0                                                     # int32 / weak float -> float32
    assert q.dtype == np.float32 and float(q) == float(f32(3) / f32(6))
    assert (1 * i).dtype == np.int32 and jnp.int16(i).dtype == np.int16 and jnp.int16(0.0).dtype == np.int16
    assert jnp.where(x > 1.5, x, 1000000).dtype == np.float32
    assert jnp.where(x > 1.5, 1.0, 0.0).dtype == np.float32
    assert jnp.array([0, -x[1], x[0]]).dtype == np.float32
    assert jnp.tile(0.02, 3).dtype == np.float32 and np.asarray(jnp.tile(0.02, 3)).tolist() == [float(f32(0.02))] * 3
    assert (x[0] >= jnp.linspace(0, 12, 3)).dtype == np.bool_
    with pytest.raises(AttributeError):
        jnp.einsum
    with pytest.raises(AttributeError):
        mods["jax"].grad
    with pytest.raises(IndexError):
        x[2]


def test_float64_mode(mods):
    jnp = mods["jax.numpy"]
    js.set_default_float(np.float64)
    try:
        assert jnp.array(0.1).dtype == np.float64 and jnp.zeros(2).dtype == np.float64
        assert jnp.float32(0.1).dtype == np.float32 and (jnp.float32(0.1) + jnp.array([0.1])).dtype == np.float64
        z = mods["jax.random"].normal(jro.prng_key(3), (4, 2))
        assert z.dtype == np.float64
        np.testing.assert_array_equal(np.asarray(z), jro.normal(jro.prng_key(3), (4, 2)).astype(np.float64))
    finally:
        js.set_default_float(np.float32)


def test_vmap_in_axes(mods):
    jax, jnp = mods["jax"], mods["jax.numpy"]

    def f(a, b, row, d):
        return jnp.sum(a * row) + b - d[0]

    a, b, d = jnp.array([1.0, 2.0, 3.0]), 0.5, jnp.array([4.0])
    rows = jnp.array(np.arange(12, dtype=np.float32).reshape(4, 3))
    got = jax.jit(jax.vmap(f, in_axes=(None, None, 0, None), out_axes=0), device=jax.devices("cpu")[0])(a, b, rows, d)
    want = np.asarray(rows) @ np.array([1, 2, 3], f32) + f32(0.5) - f32(4)
    assert got.shape == (4,) and got.dtype == np.float32
    np.testing.assert_array_equal(np.asarray(got), want)
    with pytest.raises(NotImplementedError):
        jax.vmap(f, in_axes=(None, None, 1, None))(a, b, rows, d)


def test_fori_loop_carry(mods):
    jax, jnp = mods["jax"], mods["jax.numpy"]
    seen = []

    def body(n, carry):
        total, vec = carry
        seen.append((int(n), n.dtype))
        return total + n, vec.at[n].set(total)

    total, vec = jax.lax.fori_loop(1, 5, body, (jnp.float32(0.0), jnp.zeros(5)))
    assert [s[0] for s in seen] == [1, 2, 3, 4] and all(s[1] == np.int32 for s in seen)
    assert float(total) == 10.0 and total.dtype == np.float32
    np.testing.assert_array_equal(np.asarray(vec), [0, 0, 1, 3, 6])


def test_nanargmin_first_on_ties_and_stable_argsort(mods):
    jnp = mods["jax.numpy"]
    c = jnp.array([np.nan, 5.0, 2.0, 7.0, 2.0, 2.0])
    assert int(jnp.nanargmin(c)) == 2 == int(np.nanargmin(np.asarray(c)))
    assert float(c.take(jnp.nanargmin(c))) == 2.0
    np.testing.assert_array_equal(np.asarray(jnp.argsort(jnp.array([3.0, 1.0, 3.0, 1.0, 0.0]))), [4, 1, 3, 0, 2])


def test_cov_rowvar_default(mods):
    jnp = mods["jax.numpy"]
    rng = np.random.default_rng(0)
    x = rng.standard_normal((10, 4)).astype(f32)
    got_default, got_cols = jnp.cov(jnp.array(x.T)), jnp.cov(jnp.array(x), rowvar=False)
    assert got_default.shape == (4, 4) and got_default.dtype == np.float32
    np.testing.assert_array_equal(np.asarray(got_default), np.asarray(got_cols))
    np.testing.assert_allclose(np.asarray(got_default), np.cov(x.T.astype(np.float64)), rtol=2e-6, atol=2e-6)
    assert jnp.cov(jnp.array(x)).shape == (10, 10)                  # rows are the variables by default


def test_random_is_the_threefry_restatement(mods):
    rnd = mods["jax.random"]
    key = rnd.PRNGKey(42)
    np.testing.assert_array_equal(np.asarray(key), jro.prng_key(42))
    np.testing.assert_array_equal(np.asarray(rnd.split(key)), jro.split(jro.prng_key(42), 2))
    np.testing.assert_array_equal(np.asarray(rnd.normal(key=key, shape=(5, 3))), jro.normal(jro.prng_key(42), (5, 3)))
    np.testing.assert_array_equal(np.asarray(rnd.uniform(key=key, minval=-10, maxval=10, shape=(4, 3))),
                                  jro.uniform(jro.prng_key(42), (4, 3), -10, 10))
    a = np.array([1.4, 2.0, 2.4], f32)
    np.testing.assert_array_equal(np.asarray(rnd.choice(key, mods["jax.numpy"].array([1.4, 2.0, 2.4]), shape=(9,))),
                                  jro.choice(jro.prng_key(42), a, 9))
    np.testing.assert_array_equal(np.asarray(rnd.randint(key, (6,), minval=-2, maxval=2)),
                                  jro.randint(jro.prng_key(42), 6, -2, 2))
