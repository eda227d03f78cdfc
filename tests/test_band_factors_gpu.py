"""GPU: the band kernel's B = R_A^-1 factor (band_b.h: bt_idx, BandBAdd, bt_mul, bt_tmul,
wave_prefix_sum, band_drop_b, BandMark) one update at a time, through
tests/device_units/libmpct_band_probe.so, against tests/band_factor_ref.py.  One launch per (size,
full_ri, seed); J starts as R^-1 (or its diagonal), the packed B and the two staging vectors start filled
with NaN, R_A's pointer is null (RANone).

After every script entry (band_factor_ref.check_entry, the function the CPU negative controls use):
  * q, nrot, ww, uw, the act bits of the box ids and the bitmap words of the output-row ids: exact;
  * no NaN in J, beta, w, lam or the active block of B; B's stored entries (k + 1, k), k < q, are +-0
    (row 64 has no lane, so entry (64, 63) of the full 64 x 64 block is neither written nor read);
  * in numpy.longdouble on the dumped J and B, with R_A the upper triangle of the top q x q block of
    J'N_A: |J J' - H^-1| / |H^-1|, the strictly lower part of J'N_A / |R_A| and |B R_A - I|, each
    within 8 x the float64 restatement's own worst residual over the script, never below Mz eps;
  * w = bt_tmul(B, c) and lam = bt_mul(B, w) within (ceil(q / 2) + 1) eps sum|terms| of the longdouble
    products of the dumped B (two fma chains and one add), lanes >= q exactly 0;
  * beta of an add within 64 Mz eps of the restatement's, relative.
Measured maxima are recorded in DESIGN.md, not here."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import band_factor_ref as R
from test_qp_units_gpu import families, same_bits

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_units", "libmpct_band_probe.so")
NAN = math.nan
PREFIX_FAMILIES = ("normal", "integer", "cancel", "zeros", "denormal", "each_lane")
RUNS = [(maxm, Mz, full_ri, seed) for maxm, Mz, full_ri in R.RUNS for seed in R.SEEDS]


@pytest.fixture(scope="module")
def gpu(built, has_gpu):
    if not has_gpu:
        pytest.skip("no GPU")
    return True


@pytest.fixture(scope="module")
def probe(gpu):
    return C.CDLL(LIB)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def run_band(lib, maxm, case):
    """probe_band_factors on one script: per entry the dict that band_factor_ref.check_entry takes."""
    Mz, script = case["Mz"], np.ascontiguousarray(case["script"], np.int32)
    ns, rasz = len(script), R.packed_size(Mz)
    J, B = np.full((ns, Mz * Mz), NAN), np.full((ns, rasz), NAN)
    ld, li = np.full((ns, 3, 64), NAN), np.full((ns, 2, 64), -9, np.int32)
    bw = np.full((ns, R.BIT_WORDS), 0xFFFFFFFF, np.uint32)
    sc, bt = np.full((ns, 2), -9, np.int32), np.full(ns, NAN)
    rinv, rhs = np.ascontiguousarray(case["rinv"]), np.ascontiguousarray(case["rhs"])
    normals, ids = np.ascontiguousarray(case["normals"]), np.ascontiguousarray(case["ids"], np.int32)
    rc = lib.probe_band_factors(C.c_int(maxm), C.c_int(Mz), C.c_int(case["full_ri"]), _p(rinv), C.c_int(len(ids)),
                                _p(normals), _p(ids), C.c_int(case["base"]), _p(script), C.c_int(ns), _p(rhs),
                                _p(J), _p(B), _p(ld), _p(li), _p(bw), _p(sc), _p(bt))
    assert rc == 0, (maxm, Mz, rc)
    return [dict(J=J[e], B=B[e], uw=ld[e, 0], w=ld[e, 1], lam=ld[e, 2], ww=li[e, 0], act=li[e, 1], bits=bw[e],
                 q=sc[e, 0], nrot=sc[e, 1], beta=bt[e]) for e in range(ns)]


BAND_RATIOS = {}


@pytest.mark.parametrize("maxm,Mz,full_ri,seed", RUNS, ids=lambda v: str(v))
def test_band_factor_updates(probe, maxm, Mz, full_ri, seed, capsys):
    """Adds through gi_add<MAXM>(.., RANone{}, BandBAdd) and drops through band_drop_b on one seeded
    script: a drop from q == 1, the fill to q == Mz, drops at 0, at q - 1 and at every kd of 15, 16, 31,
    32, 47, 48 below q with re-adds, then 2 Mz random adds and drops (band_factor_ref.band_script)."""
    case = R.band_case(Mz, full_ri, seed)
    out = run_band(probe, maxm, case)
    ratios = BAND_RATIOS.setdefault("band<%d>" % maxm, {})
    for e in range(len(case["script"])):
        R.check_entry(case, e, out[e], ratios)
    with capsys.disabled():
        print("\n  band factor ratios so far (jj, ra, b: device / restatement; w, lam, beta: error / bound):",
              {k: {n: round(v, 3) for n, v in sorted(r.items())} for k, r in sorted(BAND_RATIOS.items())})


def test_probe_rejects_bad_arguments(probe):
    """Arguments are validated on the host before any launch: hipErrorInvalidValue (1), no kernel run."""
    case = R.band_case(5, 1, 1)
    Mz = 5
    rinv, rhs = np.ascontiguousarray(case["rinv"]), np.ascontiguousarray(case["rhs"])
    normals, ids = np.ascontiguousarray(case["normals"]), np.ascontiguousarray(case["ids"], np.int32)

    def call(maxm=16, full=1, ids=ids, script=((0, 0), (1, 0))):
        script = np.ascontiguousarray(script, np.int32)
        ns = len(script)
        J, B = np.zeros((ns, Mz * Mz)), np.zeros((ns, R.packed_size(Mz)))
        ld, li = np.zeros((ns, 3, 64)), np.zeros((ns, 2, 64), np.int32)
        bw, sc, bt = np.zeros((ns, R.BIT_WORDS), np.uint32), np.zeros((ns, 2), np.int32), np.zeros(ns)
        return probe.probe_band_factors(C.c_int(maxm), C.c_int(Mz), C.c_int(full), _p(rinv), C.c_int(len(ids)),
                                        _p(normals), _p(ids), C.c_int(case["base"]), _p(script), C.c_int(ns),
                                        _p(rhs), _p(J), _p(B), _p(ld), _p(li), _p(bw), _p(sc), _p(bt))

    assert call() == 0
    assert call(maxm=48) == 1 and call(full=2) == 1
    assert call(script=((1, 0),)) == 1                          # a drop from the empty set
    assert call(script=((0, 0), (1, 1))) == 1                   # a drop position past q
    assert call(script=((0, len(ids)),)) == 1                   # a row past the table
    assert call(script=tuple((0, k) for k in range(Mz + 1))) == 1   # more adds than Mz
    bad = ids.copy()
    bad[3] = case["base"] + 32 * R.BIT_WORDS                    # an id past the probe's bitmap
    assert call(ids=bad) == 1
    assert probe.probe_band_prefix(C.c_int(0), _p(rhs), _p(rhs)) == 1


def prefix(lib, v):
    v = np.ascontiguousarray(v, np.float64).reshape(-1, 64)
    out = np.full(v.shape, NAN)
    rc = lib.probe_band_prefix(C.c_int(v.shape[0]), _p(v), _p(out))
    assert rc == 0, rc
    return out


def test_wave_prefix_sum(probe):
    """wave_prefix_sum on 64 lanes: exact on integer-valued inputs; elsewhere lane j within
    7 eps sum_{i <= j} |v_i| of the exact prefix (four in-row stages plus three row carries); a NaN in
    lane j0 (0, 15, 16, 63) makes lanes >= j0 NaN and leaves lanes < j0 bitwise equal to the same input
    without it."""
    fam = families()
    for name in PREFIX_FAMILIES:
        v = fam[name]
        out = prefix(probe, v)
        for c in range(v.shape[0]):
            assert R.prefix_check(out[c], v[c]), (name, c)
            if name in ("integer", "zeros", "denormal"):
                assert out[c].tolist() == R.prefix_exact(v[c]), (name, c)
    base = fam["normal"]
    clean = prefix(probe, base)
    for j0 in (0, 15, 16, 63):
        v = base.copy()
        v[:, j0] = NAN
        out = prefix(probe, v)
        assert np.isnan(out[:, j0:]).all(), j0
        assert same_bits(out[:, :j0], clean[:, :j0]), j0
