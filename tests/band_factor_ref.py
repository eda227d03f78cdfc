"""Plain reference for the probes of band_b.h (tests/device_units/band_probe.hip): the band kernel's
B = R_A^-1 factor one update at a time.  numpy and python only; tests/qp_unit_ref.py supplies make_R,
EPS, LD, normal_of and factor_tolerance.

  * BandFactorRef: a float64 restatement with general normals.  The add is FactorRef.add's (one
    Householder reflector on J(:, q:), B gains the column [-B d(0:q) / alpha; 1 / alpha]); the drop is
    restated as band_drop_b does it: rotations of the columns (jj, jj + 1), jj = kd .. q - 2, chosen to
    turn row kd of B into a multiple of e_{q-1}, applied to J's and B's columns, then row kd and the
    last column of B removed.  It is the yardstick for rounding, not the truth.
  * the truth: the invariants, evaluated in numpy.longdouble on whatever J and B are handed in
    (band_residuals), the two products against the longdouble product of the same B, and the exact
    bookkeeping (check_entry: the one function the GPU test and the CPU negative controls assert with).
  * the seeded case generator (band_case), shared by tests/test_band_factors.py (CPU: every case has
    the properties it is named for) and tests/test_band_factors_gpu.py (GPU).

Argument layouts of probe_band_factors(maxm, Mz, full_ri, rinv, nrows, normals, ids, base, script,
nscript, rhs, outJ, outB, out_lane_d, out_lane_i, out_bits, out_scal, out_beta): rinv [Mz, Mz] row-major
upper R^-1 (full_ri = 0 takes its diagonal); normals [nrows, Mz]; ids [nrows] int32; script [nscript, 2]
int32 (kind, arg): kind 0 adds row arg of normals, kind 1 drops position arg; rhs [64].  Per script
entry: outJ [Mz * Mz] = J' (J(i, k) at k * Mz + i), outB the packed array [Mz (Mz + 3) / 2] (column k
holds rows 0 .. k + 1 at k (k + 3) / 2 + row), out_lane_d [3, 64] uw, w, lam, out_lane_i [2, 64] ww, act,
out_bits [BIT_WORDS] uint32, out_scal [2] q, nrot, out_beta [1].  probe_band_prefix(ncase, in, out):
[ncase, 64] doubles each."""
import functools
import math
from fractions import Fraction

import numpy as np

import qp_unit_ref as Q

EPS, LD = Q.EPS, Q.LD
BIT_WORDS = 8          # band_probe.hip kBitWords: output-row ids base .. base + 32 * BIT_WORDS - 1
COND_CAP = 1e4         # every active set along every script: cond(R_A) <= COND_CAP, by the reference
# beta of an add: |dev - restatement| <= BETA_RULE Mz eps max(both), test_qp_units_gpu.check_factors' rule.
# beta = |J(:, q:)'n|^2 loses digits when n lies close to the active normals' span, more than cond(R_A)
# alone tells, so the generator also caps every add's amplification (add_amplification), and every case
# is held, on the CPU, to beta_margin <= 1/2: the float64 restatement's own beta is within half the rule
# of the same updates run in longdouble.  A device of the restatement's accuracy then meets the rule
BETA_RULE = 64
AMP_PER_MZ = 16.0      # every add: add_amplification <= AMP_PER_MZ * Mz (the reason is given there)
BOUNDARY_DROPS = (15, 16, 31, 32, 47, 48)   # kd around the 16-lane rows' edges

# (MAXM, Mz): the smallest sizes that reach every branch; (64, 46) is config 3's.  NU: the moves per MV
# block of the box rows on M = Mz - 1 moves (M % NU == 0)
SIZES = [(16, 2), (16, 5), (16, 16), (32, 17), (32, 32), (64, 33), (64, 46), (64, 64)]
NU = {2: 1, 5: 2, 16: 5, 17: 4, 32: 31, 33: 8, 46: 15, 64: 9}
DIAG_SIZES = [(16, 5), (32, 17), (64, 46)]   # one size per MAXM also runs with full_ri = 0
SEEDS = (1, 2)
# (Mz, seed) whose default seeds give a script that cannot keep the two caps (band_script raises) get
# other seeds here, for the rows or for R (at Mz = 2 the rule for beta is 128 eps, and R's seed 9102 has
# cond(R) = 300; 9205 has 10); no case is skipped
ROW_SEED = {(2, 1): 77420, (5, 2): 77451, (33, 1): 77730}
R_SEED = {(2, 2): 9205}
RUNS = [(maxm, Mz, 1) for maxm, Mz in SIZES] + [(maxm, Mz, 0) for maxm, Mz in DIAG_SIZES]


# ---------------------------------------------------------------------------------------------
# the packed layout (band_b.h bt_idx, gi_core.h ra_packed_size)
def packed_size(Mz):
    return Mz * (Mz + 3) // 2


def bt_idx(w, k):
    return k * (k + 3) // 2 + w


def unpack_b(packed, q):
    """The upper triangle of the active block, B(w, k) for w <= k < q."""
    B = np.zeros((q, q))
    for k in range(q):
        B[:k + 1, k] = packed[bt_idx(0, k):bt_idx(0, k) + k + 1]
    return B


def pack_b(B, Mz):
    """B's upper triangle in the packed array, the stored subdiagonal (k + 1, k), k < q, zero and
    every other entry NaN: what a launch that starts from a NaN-filled array must leave."""
    q = B.shape[0]
    out = np.full(packed_size(Mz), np.nan)
    for k in range(q):
        out[bt_idx(0, k):bt_idx(0, k) + k + 1] = B[:k + 1, k]
        out[bt_idx(k + 1, k)] = 0.0
    return out


# ---------------------------------------------------------------------------------------------
# the float64 restatement
class BandFactorRef:
    """H^-1 = J J', J'N_A = [R_A; 0], B = R_A^-1, in `dtype` arithmetic (float64: the restatement;
    numpy.longdouble: what band_case measures the restatement's beta against).  `flip` / `slot` (negative
    controls only): the index of one rotation whose sine is negated on J, and the index of one rotating
    drop after which the row of B that moved up into place kd is written one slot to the right."""

    def __init__(self, J0, flip=None, slot=None, dtype=np.float64):
        self.Mz, self.dt = J0.shape[0], dtype
        self.J = np.array(J0, dtype)
        self.B = np.zeros((0, 0), dtype)
        self.ww, self.uw, self.rows = [], [], []
        self.nrot, self.nrotation, self.ndrop, self.flip, self.slot = 0, 0, 0, flip, slot

    def add(self, row, p, n, upm):
        q, J = len(self.ww), self.J
        d = J.T @ np.asarray(n, self.dt)
        beta = d[q:] @ d[q:]
        nrm = np.sqrt(beta)
        alpha = -nrm if d[q] > 0.0 else nrm
        v = d[q:].copy()
        v[0] -= alpha
        f = (J[:, q:] @ d[q:] - alpha * J[:, q]) / (beta - alpha * d[q])
        J[:, q:] -= np.outer(f, v)
        B = np.zeros((q + 1, q + 1), self.dt)
        B[:q, :q] = self.B
        B[:q, q] = -(self.B @ d[:q]) / alpha
        B[q, q] = 1 / alpha
        self.B = B
        self.ww.append(p)
        self.uw.append(float(upm))
        self.rows.append(row)
        self.nrot += 1
        return beta

    def drop(self, kd):
        q, B, J = len(self.ww), self.B.copy(), self.J
        for jj in range(kd, q - 1):
            x, y = B[kd, jj], B[kd, jj + 1]
            r = np.sqrt(x * x + y * y)
            cs, sn = (y / r, -x / r) if r > 0.0 else (self.dt(1), self.dt(0))
            G = np.array([[cs, sn], [-sn, cs]], self.dt)
            B[:, jj:jj + 2] = B[:, jj:jj + 2] @ G.T
            if self.flip == self.nrotation:
                G = np.array([[cs, -sn], [sn, cs]], self.dt)
            J[:, jj:jj + 2] = J[:, jj:jj + 2] @ G.T
            self.nrotation += 1
        B = np.triu(np.delete(B, kd, axis=0)[:, :q - 1])
        if kd < q - 1:
            if self.slot == self.ndrop:
                B[kd, 1:] = B[kd, :-1].copy()
                B[kd, 0] = 0.0
            self.ndrop += 1
        self.B = B
        self.nrot += q - 1 - kd
        del self.ww[kd], self.uw[kd], self.rows[kd]


def band_residuals(Hi, N_A, J, B):
    """The invariants of one state in numpy.longdouble, each a relative residual (Frobenius norms), with
    R_A the upper triangle of the top q x q block of J'N_A:  jj: |J J' - H^-1| / |H^-1|;  ra: the
    strictly lower part of J'N_A over all Mz rows (so: upper triangular, zero below row q) / |R_A|;
    b: |B R_A - I|."""
    Jl = np.asarray(J, LD)
    Hl = np.asarray(Hi, LD)
    out = dict(jj=float(np.linalg.norm(Jl @ Jl.T - Hl) / np.linalg.norm(Hl)))
    q = N_A.shape[1]
    if q:
        JN = Jl.T @ np.asarray(N_A, LD)
        Ru = np.triu(JN[:q])
        out["ra"] = float(np.linalg.norm(np.tril(JN, -1)) / np.linalg.norm(Ru))
        out["b"] = float(np.linalg.norm(np.asarray(B, LD) @ Ru - np.eye(q, dtype=LD)))
    return out


# ---------------------------------------------------------------------------------------------
# cases
def make_rows(Mz, seed):
    """(normals [nrows, Mz], ids [nrows], base), nrows = 3 Mz: one box row of gi_core.h's cinfo per move
    of the M = Mz - 1 moves (rate kinds 0 / 1, amplitude kinds 2 / 3 off the block's first move), the eps
    row e_M (id 4 M), and Mz upper / lower pairs of dense output rows [-g, v_u], [+g, v_l] (v > 0, the
    pair sharing g as the kernel's rows do) with ids base + 2 r, base + 2 r + 1, base = 4 Mz.  The r
    include 15, 16 (bits 31 | 32 of the bitmap) and, from Mz = 5, 31, 32 (bits 63 | 64)."""
    rng = np.random.default_rng(ROW_SEED.get((Mz, seed), 77000 + 100 * Mz + seed))
    M, Nu, base = Mz - 1, NU[Mz], 4 * Mz
    normals, ids = [], []
    for m in range(M):
        kind = int(rng.choice([0, 1] + ([2, 3] if m % Nu else [])))
        normals.append(np.append(Q.normal_of(4 * m + kind, M, Nu), 0.0))
        ids.append(4 * m + kind)
    normals.append(np.eye(Mz)[M])
    ids.append(4 * M)
    forced = [15, 16] + ([31, 32] if Mz >= 5 else [])
    rest = [r for r in range(32 * BIT_WORDS // 2) if r not in forced]
    rs = sorted(forced + [int(r) for r in rng.permutation(rest)[:Mz - len(forced)]])
    for r in rs:
        g = rng.standard_normal(M) * rng.uniform(0.5, 2.0) / math.sqrt(M)
        vu, vl = rng.uniform(0.3, 1.5, 2)
        normals += [np.append(-g, vu), np.append(g, vl)]
        ids += [base + 2 * r, base + 2 * r + 1]
    return np.array(normals), np.array(ids, np.int32), base


def set_cond(Ji, normals, rows):
    """cond(R_A) of the active set `rows`: R_A'R_A = N_A'H^-1 N_A, so R_A's singular values are those
    of J0'N_A for the starting J0 (H^-1 = J0 J0')."""
    if not rows:
        return 1.0
    s = np.linalg.svd(Ji.T @ normals[list(rows)].T, compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0.0 and len(rows) <= Ji.shape[0] else math.inf


def add_amplification(Ji, normals, act, r):
    """|J|_F |n| / |J(:, q:)'n| for the add of row r to the active rows `act`, from the starting J0 alone
    (J(:, q:) = J0 Q2, Q2 an orthonormal basis of the complement of J0'N_A's range; |J|_F = |J0|_F):
    how much the add's beta = |J(:, q:)'n|^2 magnifies rounding.  The reflectors and rotations mix J's
    columns, so each column carries an error of about c eps |J|_F, d_k = J(:, k)'n one of c eps |J|_F |n|,
    and beta a relative error of 2 c eps times this figure, c a small multiple of one.  The rule for beta
    (BETA_RULE Mz eps) then needs the figure below 32 Mz / c; AMP_PER_MZ = 16 leaves c a factor of two
    (the float64 restatement against its longdouble twin, band_case's beta_margin, shows c near 0.4)."""
    q, n = len(act), normals[r]
    Q2 = np.linalg.qr(Ji.T @ normals[list(act)].T, mode="complete")[0][:, q:] if q else np.eye(Ji.shape[0])
    nrm = float(np.linalg.norm(Q2.T @ (Ji.T @ n)))
    return float(np.linalg.norm(Ji) * np.linalg.norm(n) / nrm) if nrm > 0.0 else math.inf


def band_script(Mz, Ji, normals, ids, base, seed):
    """[(kind, arg)]: kind 0 adds row arg of `normals`, kind 1 drops position arg.  An add takes the
    first row, in a seeded order, that keeps cond(R_A) <= COND_CAP (a drop never raises it: R_A loses
    a column) and add_amplification <= AMP_PER_MZ Mz, so both caps hold along the whole script by
    construction (a re-add takes the dropped row when it passes, else the next row that does); a script that cannot go on
    raises here.  Add one row and drop it (a drop from q == 1); fill to q == Mz, the rows of bitmap bits
    31, 32 (63, 64) first; drop position 0 and re-add the row; drop q - 1 (no rotation) and re-add; drop
    at every kd of BOUNDARY_DROPS below q and re-add; then 2 Mz random adds and drops, the first add a
    box row."""
    rng = np.random.default_rng(88000 + 100 * Mz + seed)
    nrows = len(ids)
    script, act = [], []

    def add(r):
        script.append((0, int(r)))
        act.append(int(r))

    def drop(kd):
        script.append((1, int(kd)))
        return act.pop(kd)

    def pick(order):
        for r in order:
            if r not in act and add_amplification(Ji, normals, act, int(r)) <= AMP_PER_MZ * Mz and \
                    set_cond(Ji, normals, act + [int(r)]) <= COND_CAP:
                return int(r)
        raise AssertionError("no row keeps cond(R_A) <= %g and the add's amplification <= %g Mz (Mz %d, seed %d, q %d)"
                             % (COND_CAP, AMP_PER_MZ, Mz, seed, len(act)))

    first = [r for r in range(nrows) if ids[r] - base in (31, 32) + ((63, 64) if Mz >= 5 else ())]
    add(pick(rng.permutation(nrows)))
    drop(0)
    for r in first[:Mz]:
        add(pick([r]))
    while len(act) < Mz:
        add(pick(rng.permutation(nrows)))
    for kd in [0, Mz - 1] + [k for k in BOUNDARY_DROPS if k < Mz]:
        add(pick([drop(kd)] + list(rng.permutation(nrows))))
    box_first = True
    for _ in range(2 * Mz):
        if act and (len(act) == Mz or rng.random() < 0.5):
            drop(int(rng.integers(len(act))))
        else:
            order = rng.permutation(nrows)
            if box_first:
                order = [r for r in order if ids[r] < base] + [r for r in order if ids[r] >= base]
                box_first = False
            add(pick(order))
    return script


def bookkeeping(ww):
    """(act [64], bits [BIT_WORDS]) of the active ids: box ids p < base set bit p & 3 of lane p >> 2, output
    ids bit (p - base) & 31 of word (p - base) >> 5 (band_b.h BandMark).  `ww` is [(id, base)]."""
    act, bits = np.zeros(64, np.int64), np.zeros(BIT_WORDS, np.int64)
    for p, base in ww:
        if p < base:
            act[p >> 2] |= 1 << (p & 3)
        else:
            bits[(p - base) >> 5] |= 1 << ((p - base) & 31)
    return act, bits


@functools.lru_cache(maxsize=None)
def band_case(Mz, full_ri, seed, flip=None, slot=None):
    """The rows, the script, R^-1, the right-hand side of the products and the restatement's state and
    residuals after every entry."""
    rinv = np.triu(np.linalg.inv(Q.make_R(Mz, R_SEED.get((Mz, seed), 9100 + seed))))
    Ji = rinv if full_ri else np.diag(np.diag(rinv))     # the kernel's load_j
    Hi = Ji @ Ji.T
    normals, ids, base = make_rows(Mz, seed)
    rhs = np.random.default_rng(66000 + seed).standard_normal(64)
    script = band_script(Mz, Ji, normals, ids, base, seed)
    ref, states = BandFactorRef(Ji, flip, slot), []
    twin, margin = BandFactorRef(Ji, dtype=LD), 0.0      # the same updates in longdouble, for beta alone
    for e, (kind, arg) in enumerate(script):
        amp = add_amplification(Ji, normals, ref.rows, arg) if kind == 0 else 0.0
        if kind == 0:
            beta = float(ref.add(arg, int(ids[arg]), normals[arg], e + 1))
            bl = float(twin.add(arg, int(ids[arg]), normals[arg], e + 1))
            margin = max(margin, abs(beta - bl) / (BETA_RULE * Mz * EPS * max(beta, bl)))
        else:
            beta = 0.0
            ref.drop(arg)
            twin.drop(arg)
        q = len(ref.ww)
        act, bits = bookkeeping([(p, base) for p in ref.ww])
        res = band_residuals(Hi, normals[ref.rows].T.reshape(Mz, q), ref.J, ref.B)
        states.append(dict(ww=list(ref.ww), uw=list(ref.uw), rows=list(ref.rows), act=act, bits=bits, q=q,
                           nrot=ref.nrot, beta=beta, res=res, J=ref.J.copy(), B=ref.B.copy(),
                           cond=set_cond(Ji, normals, ref.rows), amp=amp))
    worst = {k: max(s["res"].get(k, 0.0) for s in states) for k in ("jj", "ra", "b")}
    return dict(M=Mz, Mz=Mz, full_ri=full_ri, seed=seed, rinv=rinv, Hi=Hi, normals=normals, ids=ids, base=base,
                rhs=rhs, script=script, states=states, ref_worst=worst, beta_margin=margin)


def tolerance(case, key):
    """The project's rule (qp_unit_ref.factor_tolerance): 8 x the restatement's own worst residual over
    the script, never below Mz eps."""
    return Q.factor_tolerance(case, key)


# ---------------------------------------------------------------------------------------------
# the check of one dumped state
def product_bound(q, terms):
    """|dev - exact| <= (ceil(q / 2) + 1) eps sum|terms|: bt_mul / bt_tmul run two fma chains of at most
    ceil(q / 2) terms each (one rounding per fma, each relative eps / 2 of a partial sum bounded by
    sum|terms|) and add them once."""
    return ((q + 1) // 2 + 1) * LD(EPS) * np.abs(terms).sum(axis=1)


def restated_entry(case, e):
    """State e of the restatement in the form the probe dumps it (the input of check_entry): J' flat,
    the packed B with NaN wherever no add or drop writes, the lane vectors, w = B'c and lam = B w rounded
    from longdouble."""
    st, Mz = case["states"][e], case["Mz"]
    q = st["q"]
    uw, ww = np.zeros(64), np.full(64, -1, np.int64)
    uw[:q], ww[:q] = st["uw"], st["ww"]
    w, lam = np.zeros(64), np.zeros(64)
    w[:q] = (np.asarray(st["B"], LD).T @ np.asarray(case["rhs"][:q], LD)).astype(float)
    lam[:q] = (np.asarray(st["B"], LD) @ np.asarray(w[:q], LD)).astype(float)
    return dict(J=st["J"].T.reshape(-1).copy(), B=pack_b(st["B"], Mz), uw=uw, ww=ww, act=st["act"].copy(),
                bits=st["bits"].copy(), q=q, nrot=st["nrot"], beta=st["beta"], w=w, lam=lam)


def check_entry(case, e, dev, ratios=None):
    """Everything asserted about the state after script entry e.  `dev`: J [Mz * Mz] (J', as dumped), B the
    packed array, uw, w, lam, ww, act [64], bits [BIT_WORDS], q, nrot, beta.  Returns the residuals; with
    `ratios` (a dict) keeps the worst residual / restatement's worst per invariant."""
    st, Mz, base = case["states"][e], case["Mz"], case["base"]
    kind, arg = case["script"][e]
    tag = ("Mz %d full_ri %d seed %d entry %d" % (Mz, case["full_ri"], case["seed"], e), (kind, arg))
    q = st["q"]
    # bookkeeping, exact
    assert int(dev["q"]) == q and int(dev["nrot"]) == st["nrot"], tag + (int(dev["q"]), int(dev["nrot"]), st["nrot"])
    ww, uw = np.asarray(dev["ww"]), np.asarray(dev["uw"])
    assert ww[:q].tolist() == st["ww"] and np.all(ww[q:] == -1), tag + (ww.tolist(),)
    assert uw[:q].tolist() == st["uw"] and np.all(uw[q:] == 0.0), tag + (uw.tolist(),)
    assert np.array_equal(np.asarray(dev["act"], np.int64), st["act"]), tag
    assert np.array_equal(np.asarray(dev["bits"], np.int64), st["bits"]), tag + (np.asarray(dev["bits"]).tolist(),)
    # no NaN in J, beta or the active block of B; the stored subdiagonal (k + 1, k), k < q, is +-0.  Row
    # 64 has no lane: at q == Mz == 64 nothing writes or reads entry (64, 63), the one entry left out
    J = np.asarray(dev["J"], float).reshape(Mz, Mz).T
    packed = np.asarray(dev["B"], float)
    assert packed.shape == (packed_size(Mz),), tag
    assert np.all(np.isfinite(J)) and math.isfinite(float(dev["beta"])), tag
    for k in range(q):
        col = packed[bt_idx(0, k):bt_idx(0, k) + k + 1]
        assert np.all(np.isfinite(col)), tag + ("B column", k)
        if k + 1 < 64:
            assert packed[bt_idx(k + 1, k)] == 0.0, tag + ("B subdiagonal", k, packed[bt_idx(k + 1, k)])
    B = unpack_b(packed, q)
    # the invariants
    res = band_residuals(case["Hi"], case["normals"][st["rows"]].T.reshape(Mz, q), J, B)
    for k, v in res.items():
        tol = tolerance(case, k)
        assert v <= tol, tag + (k, v, tol)
        if ratios is not None:
            ratios[k] = max(ratios.get(k, 0.0), v / max(case["ref_worst"][k], 1e-300))
    # the products, against the longdouble products of this same B
    w, lam = np.asarray(dev["w"], float), np.asarray(dev["lam"], float)
    assert np.all(w[q:] == 0.0) and np.all(lam[q:] == 0.0), tag
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(lam)), tag
    if q:
        Bl, c = np.asarray(B, LD), np.asarray(case["rhs"][:q], LD)
        tw = Bl.T * c[None, :]                  # row v: B(k, v) c_k
        tl = Bl * np.asarray(w[:q], LD)[None, :]   # row r: B(r, k) w_k
        for name, got, terms in (("w", w, tw), ("lam", lam, tl)):
            err = np.abs(np.asarray(got[:q], LD) - terms.sum(axis=1))
            bound = product_bound(q, terms)
            assert np.all(err <= bound), tag + (name, float((err / np.maximum(bound, LD(1e-300))).max()))
            if ratios is not None:
                ratios[name] = max(ratios.get(name, 0.0), float((err / np.maximum(bound, LD(1e-300))).max()))
    # beta: the rule of test_qp_units_gpu.check_factors
    if q and kind == 0:
        if ratios is not None:
            ratios["beta"] = max(ratios.get("beta", 0.0), abs(float(dev["beta"]) - st["beta"]) /
                                 (BETA_RULE * Mz * EPS * max(st["beta"], float(dev["beta"]))))
        assert abs(float(dev["beta"]) - st["beta"]) <= BETA_RULE * Mz * EPS * max(st["beta"], float(dev["beta"])), \
            tag + ("beta", float(dev["beta"]), st["beta"])
    return res


# ---------------------------------------------------------------------------------------------
# wave_prefix_sum
def prefix_check(dev, v):
    """Lane j within 7 eps sum_{i <= j} |v_i| of the exact prefix (rational arithmetic): four in-row
    stages and three row carries, each one rounded addition."""
    fr = [Fraction(float(x)) for x in v]
    s, a = Fraction(0), Fraction(0)
    for j in range(64):
        s += fr[j]
        a += abs(fr[j])
        if abs(Fraction(float(dev[j])) - s) > 7 * Fraction(EPS) * a:
            return False
    return True


def prefix_exact(v):
    return [math.fsum(v[:j + 1]) for j in range(64)]
