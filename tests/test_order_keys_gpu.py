"""The dispatch-order keys and permutation on the device (csrc/work_order.hip through
tests/device_units/order_probe.hip) against the exact reference of tests/order_key_ref.py, under its
comparison rule: M bits and fixed values equal, the field inside the candidate's rounding window, which
holds one integer for all but at most 2 % of a batch (tests/test_order_keys.py asserts that, the
condition bound and that every batch reaches the path it is named for, on the CPU).  The permutation
must be the stable ascending sort of the device keys."""
import numpy as np
import pytest

import order_key_ref as R

pytestmark = pytest.mark.gpu

_RUNS = {}


@pytest.fixture(scope="module")
def probe(built):
    return R.Probe()


def _run(probe, name):
    """(keys, perm) of a batch, one probe call per batch and module."""
    if name not in _RUNS:
        b = R.BATCHES[name]
        desc, keep = b.desc()
        _RUNS[name] = probe.order(desc, R.K_GPC, *b.candidates(), refs=b.r, tables=b.tables)
        del keep
    return _RUNS[name]


def _check(keys, perm, ref, what):
    bad = R.compare(keys, ref)
    inv = ~keys
    print("%s: %d candidates, %d valid, %d outside the rule" % (what, keys.size, int(ref.valid.sum()), int(bad.sum())))
    for c in np.flatnonzero(bad)[:8]:
        print("  c=%d device key %08x (M %d field %d) reference %08x window [%d, %d] fixed %d x %.6f dx %.3g" % (
            c, keys[c], inv[c] >> 20, inv[c] & R.FIELD_MAX, ref.key[c], ref.lo[c], ref.hi[c], ref.fixed[c],
            float(ref.x[c]), ref.dx[c]))
    assert not bad.any(), what
    assert np.array_equal(perm, np.argsort(keys, kind="stable")), what + ": permutation"


@pytest.mark.parametrize("name", list(R.BATCHES))
def test_keys_and_order_of_batch(probe, name):
    keys, perm = _run(probe, name)
    _check(keys, perm, R.BATCHES[name].reference(), name)


@pytest.mark.parametrize("tabled, dropped", (("shell-steps", "shell-lds"), ("siso", "siso-lds"), ("4x3", "4x3-lds")))
def test_lds_built_h_agrees_with_the_tables(probe, tabled, dropped):
    """The same candidates with and without the Gram tables: both keys lie in the candidate's window, so
    they are equal wherever it holds one integer."""
    a, b = R.BATCHES[tabled], R.BATCHES[dropped]
    assert all(np.array_equal(x, y) for x, y in zip(a.candidates(), b.candidates())) and not b.tables
    ref = a.reference()
    ka, kb = _run(probe, tabled)[0], _run(probe, dropped)[0]
    one = ref.lo == ref.hi
    print("%s / %s: %d keys differ" % (tabled, dropped, int((ka != kb).sum())))
    assert not R.compare(ka, ref).any() and not R.compare(kb, ref).any()
    assert np.array_equal(ka[one], kb[one])


@pytest.mark.parametrize("kind", (R.K_GPC, R.K_NMPC))
@pytest.mark.parametrize("my, nu", ((3, 3), (2, 1), (1, 2)))
def test_keys_without_a_scenario(probe, kind, my, nu):
    """order_keys: the weight-ratio key and the NMPC key (no descriptor)."""
    cand = R.null_candidates(my, nu, C=256 + (my & 1), seed=70 + my)
    keys, perm = probe.order(None, kind, *cand, my=my, nu=nu)
    _check(keys, perm, R.ratio_reference(kind, my, nu, *cand), "no scenario, kind %d, my %d, nu %d" % (kind, my, nu))


@pytest.mark.parametrize("C", R.LARGE_C)
def test_order_on_both_sides_of_the_counting_rank(probe, C):
    """A 257-candidate batch of the tabled Shell 3x3 path tiled to C: many ties, the counting rank up
    to kCountRankMaxC and the radix sort above."""
    b = R.BATCHES["shell-steps"]
    cand, ref = R.tiled(b, C)
    desc, keep = b.desc()
    keys, perm = probe.order(desc, R.K_GPC, *cand, refs=b.r)
    _check(keys, perm, ref, "shell-steps tiled to %d" % C)
    assert np.array_equal(keys, _run(probe, "shell-steps")[0][np.arange(C) % b.C])
