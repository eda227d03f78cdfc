"""Plain reference for the probe of gpc_prologue.h (tests/device_units/prologue_probe.hip): the block
Householder QR of W = [Q^1/2 G; Lambda^1/2] carrying V = [Q^1/2 Phi; 0], the gain A = -R^-1 Q1'V and R^-1.
numpy, mpmath and python only; nothing imported from the product package.

  * build_W restates MatG's indexing (entry (r, n Nu + c) of output i is step[i, n, n1[i] + r - c], zero
    for a negative index), |weight| and its square root unless wsq.
  * the truth (truth_of): Householder QR of W in mpmath at MP_DPS digits, never W'W: R with a positive
    diagonal, T = Q1'V, A* = -R^-1 T, Rinv*, cond(W).
  * the tables of the TABLES instances (mp_tables): per output G_i = Q_i R_i, T_i = Q_i'Phi_i in mpmath,
    rounded to double, rows interleaved my k + i, min(N2, M) rows per output, at the offsets of
    scenario_tables.h qr_tables (cell_offsets).
  * Restatement (restate): the same block algorithm in float64 (blocks of kHB, v0 = -sigma / (x0 + ||x||),
    streamed and table sources, the table blocks starting at level blk kHB / my).  It is the yardstick for
    rounding, not the truth; its switches are the negative controls of tests/test_prologue_units.py.
  * check_case: the one function the GPU test and the CPU negative controls assert with, on the LDS image
    the probe dumps (image_of builds the same image from the restatement).
  * the seeded cases (FAMILIES), shared by tests/test_prologue_units.py (CPU: every case has the properties
    it is named for) and tests/test_prologue_units_gpu.py.

The bounds.  u = 2^-53.  One reflection acts on the vectors [R_kj; w_.j] of length kHB + 1 as
H = I - beta v v', v = [v0; w_.k].  The device forms sigma by two fma chains (relative error a =
(kHB / 2 + 1) u), t = fma(x0, x0, sigma) (a + u), 1 / sqrt(t) by rsq_nr (2.5 ulp <= 5 u, test_rcp_rsq_ulps),
n = t rsq (theta_n = a / 2 + 6.5 u), x0 + n without cancellation (R_kk stays positive: + u), its reciprocal by
rcp_nr (1 ulp <= 2 u) and one product: theta_v = 1.5 a + 10.5 u for v0, and theta_beta = 2 a + 17 u for
beta = rsq (x0 + n) rcp(sigma).  With beta |v|^2 = 2, |H^ - H|_F <= 2 (theta_beta + 2 theta_v) = 10 a + 76 u.
Applying H^: the inner product of kHB + 1 terms (gamma_{kHB + 2} |v| |y|, times beta |v| <= 2 / |v|), f = beta s
(u, times 2) and one fma per entry (u, on at most 3 |y|): (2 (kHB + 1) + 7) u.  Together, first order,
    gamma_ref(kHB) = (7 kHB + 95) u   per reflection (Higham, Accuracy and Stability, Lemma 19.2 / 19.3 with
the constants written out), and by Theorem 19.4's column-wise form the computed [R | T] is the exact
factor of [W + dW | V + dV], |dW_:j| <= c |W_:j|, c = r gamma_ref + 6 u, r the number of reflections applied
(nblk M streamed; the table source applies sum over its blocks of M - k0) and 6 u for the rounding of the
weight's square root (2 ulp) and its product.  The table rows add their own stage to c: u when they are
rounded from mpmath, min(N2, M) gamma_ref(N2) when the host's float64 Householder built them.  Hence
    |R'R - W'W|_ij <= g |W_:i| |W_:j|,   g = 2 c + c^2,
    |R'(R A) + W'V|_ij <= g (|W_:i| |V_:j| + (|R'| |R| |A|)_ij)   (the back substitution R A = -T holds to
                                                                  gamma_M |R| |A| <= g |R| |A|),
    |R Rinv - I| <= gamma_{M + 1} |R| |Rinv|   componentwise (Higham Theorem 8.5),
    |R^_:j - R_:j| <= cond(W) g |R_:j|   (the first-order perturbation of the QR factor under dW),
and for the forward errors of A and Rinv the derived figures of forward_bounds (the least-squares bound of
Higham Theorem 20.1 with the residual from the truth).  Nothing here is tuned to a device: on the CPU
every case's restatement is held to half of every bound (tests/test_prologue_units.py).

Argument layout of probe_prologue(instance, ncase, hdr, dpool, ndbl, ipool, nint, out_lds, out_flags,
out_ldsn): hdr [ncase, len(HDR)] int32 (fields HDR; the *_off fields index dpool or ipool, -1 = absent),
out_lds [ncase, ldsn] the whole LDS image of every case (layout_of; filled with SENTINEL before the call),
out_flags [ncase, 64] the flag of every lane.  pack_launch builds the arguments."""
import functools
import math

import mpmath as mp
import numpy as np

U = 2.0 ** -53
EPS = 2.0 ** -52
LD = np.longdouble
MP_DPS = 70
SENTINEL = 0x7FF8A5C3D2E1F097   # prologue_probe.hip kSentinel
GUARD = 64                      # prologue_probe.hip kGuard
COND_CAP = 1e6
HDR = ("inst my nu nx wsq tlen n2max numax M Nu N2 astride step_off phi_off n1_off delta_off lambda_off "
       "acol_off qrt_off qrt_len qoff_off").split()

INSTANCES = {
    0: dict(name="gpc_prologue<16>", maxm=16, packed=False, rinv=True, first=False, khb=8, tables=False),
    1: dict(name="gpc_prologue<32>", maxm=32, packed=False, rinv=True, first=False, khb=8, tables=False),
    2: dict(name="gpc_prologue<64>", maxm=64, packed=False, rinv=True, first=False, khb=8, tables=False),
    3: dict(name="small<16,P,12,tables>", maxm=16, packed=True, rinv=True, first=False, khb=12, tables=True),
    4: dict(name="small<16,P,12>", maxm=16, packed=True, rinv=True, first=False, khb=12, tables=False),
    5: dict(name="dtc<16,first,4>", maxm=16, packed=False, rinv=False, first=True, khb=4, tables=False),
    6: dict(name="dtc<32,first,4>", maxm=32, packed=False, rinv=False, first=True, khb=4, tables=False),
    # the other side of a bitwise comparison only (no kernel's instance)
    7: dict(name="cmp<16,4>", maxm=16, packed=False, rinv=False, first=False, khb=4, tables=False),
    8: dict(name="cmp<32,4>", maxm=32, packed=False, rinv=False, first=False, khb=4, tables=False),
    9: dict(name="cmp<16,full,12>", maxm=16, packed=False, rinv=True, first=False, khb=12, tables=False),
}
PRODUCTION = (0, 1, 2, 3, 5, 6)


def gamma(n):
    return n * U / (1.0 - n * U)


def gamma_ref(khb):
    """The per-reflection constant derived in the module docstring."""
    return (7 * khb + 95) * U


# ---------------------------------------------------------------------------------------------
# the layout of the probe's LDS image
def layout_of(inst, M, Nu, astride):
    I = INSTANCES[inst]
    ri = M * M
    a = ri + (GUARD if not I["rinv"] else M * (M + 1) // 2 if I["packed"] else M * M)
    end = a + (M // Nu if I["first"] else M) * astride
    return dict(ri=ri, a=a, end=end, total=end + GUARD)


def rinv_idx(i, k, M, packed):
    """gpc_prologue.h ri(): entry (i, k), i <= k, of R^-1."""
    return i * M - (i * (i - 1)) // 2 + (k - i) if packed else i * M + k


# ---------------------------------------------------------------------------------------------
# W, V and the truth
def weights(w, wsq):
    w = np.abs(np.asarray(w, float))
    return w if wsq else np.sqrt(w)


def build_G(step, n1, i, N2, Nu):
    """G_i [N2, nu Nu]: MatG's indexing, tt = n1[i] + r - gc, zero for tt < 0."""
    nu = step.shape[1]
    G = np.zeros((N2, nu * Nu))
    for r in range(N2):
        for n in range(nu):
            for c in range(Nu):
                tt = int(n1[i]) + r - c
                if tt >= 0:
                    G[r, n * Nu + c] = step[i, n, tt]
    return G


def build_W(step, phi, n1, delta, lam, wsq, N2, Nu, exact=False):
    """(W [my N2 + M, M], V [my N2 + M, nx]): the rows sqrt(delta_i) [G_i | Phi_i], output-major, then
    Lambda^1/2 with zero V rows.  exact: lists of mpmath numbers, the square roots taken in mpmath."""
    my, nu = step.shape[0], step.shape[1]
    M, nx = nu * Nu, phi.shape[2]
    if exact:
        sq = [mp.mpf(abs(float(d))) if wsq else mp.sqrt(mp.mpf(abs(float(d)))) for d in delta]
        sl = [mp.mpf(abs(float(d))) if wsq else mp.sqrt(mp.mpf(abs(float(d)))) for d in lam]
    else:
        sq, sl = weights(delta, wsq), weights(lam, wsq)
    rows = []
    for i in range(my):
        G = build_G(step, n1, i, N2, Nu)
        for r in range(N2):
            if exact:
                rows.append([sq[i] * mp.mpf(float(x)) for x in G[r]] + [sq[i] * mp.mpf(float(x)) for x in phi[i, r]])
            else:
                rows.append(np.concatenate([sq[i] * G[r], sq[i] * phi[i, r]]))
    for m in range(M):
        z = [mp.mpf(0)] * (M + nx) if exact else np.zeros(M + nx)
        z = list(z) if exact else z
        z[m] = sl[m // Nu]
        rows.append(z)
    if exact:
        return [r[:M] for r in rows], [r[M:] for r in rows]
    a = np.array(rows)
    return a[:, :M], a[:, M:]


def mp_householder(a, ncols):
    """Householder QR in place on the list of rows `a`, reducing its first ncols columns; rows whose
    diagonal comes out negative are negated, so the triangle has a non-negative diagonal."""
    m, w = len(a), len(a[0])
    zero = mp.mpf(0)
    for k in range(min(ncols, m)):
        rows = [r for r in range(k + 1, m) if a[r][k] != 0]
        if rows:
            sig = mp.fsum(a[r][k] ** 2 for r in rows)
            x0 = a[k][k]
            nrm = mp.sqrt(x0 * x0 + sig)
            alpha = -nrm if x0 > 0 else nrm
            v0 = x0 - alpha
            tau = 2 / (v0 * v0 + sig)
            ak = a[k]
            for c in range(k + 1, w):
                dot = v0 * ak[c] + mp.fsum(a[r][k] * a[r][c] for r in rows)
                if dot == 0:
                    continue
                dot *= tau
                ak[c] -= dot * v0
                for r in rows:
                    a[r][c] -= dot * a[r][k]
            ak[k] = alpha
            for r in rows:
                a[r][k] = zero
        if a[k][k] < 0:
            a[k] = [-x for x in a[k]]
    return a


def to_ld(x):
    hi = float(x)
    return LD(hi) + LD(float(x - hi))


def ld_array(rows):
    return np.array([[to_ld(x) for x in r] for r in rows], LD).reshape(len(rows), -1)


def truth_of(case):
    """R, T, A*, Rinv* in numpy.longdouble (rounded from mpmath), cond(W) and the norms the bounds use."""
    key = case["key"]
    if key not in _TRUTH:
        _TRUTH[key] = _truth(case)
    return _TRUTH[key]


_TRUTH = {}


def _truth(case):
    with mp.workdps(MP_DPS):
        M, nx = case["M"], case["nx"]
        W, V = build_W(case["step"], case["phi"], case["n1"], case["delta"], case["lam"], case["wsq"], case["N2"],
                       case["Nu"], exact=True)
        vn = np.array([float(mp.sqrt(mp.fsum(V[r][j] ** 2 for r in range(len(V))))) for j in range(nx)])
        a = mp_householder([w + v for w, v in zip(W, V)], M)[:M]
        R = [[a[i][j] for j in range(M)] for i in range(M)]
        T = [[a[i][M + j] for j in range(nx)] for i in range(M)]
        ok = all(R[k][k] > 0 for k in range(M))
        out = dict(ok=ok, vn=vn, R=ld_array(R))
        if not ok:
            return out

        def solve(B):   # R X = B, columns at once
            n = len(B[0])
            X = [[mp.mpf(0)] * n for _ in range(M)]
            for kk in range(M - 1, -1, -1):
                for j in range(n):
                    s = B[kk][j] - mp.fsum(R[kk][c] * X[c][j] for c in range(kk + 1, M))
                    X[kk][j] = s / R[kk][kk]
            return X

        X = solve(T)
        Ri = solve([[mp.mpf(1 if i == j else 0) for j in range(M)] for i in range(M)])
        out.update(T=ld_array(T), A=-ld_array(X), Rinv=ld_array(Ri))
    Rf = out["R"].astype(float)
    s = np.linalg.svd(Rf, compute_uv=False)
    out.update(cond=float(s[0] / s[-1]), smax=float(s[0]), smin=float(s[-1]),
               wn=np.sqrt((out["R"] ** 2).sum(axis=0)).astype(float))
    tn2 = (out["T"] ** 2).sum(axis=0).astype(float)
    out["res"] = np.sqrt(np.maximum(vn ** 2 - tn2, 0.0))   # |V_:j - W A*_:j|, for the bound only
    return out


# ---------------------------------------------------------------------------------------------
# the tables
def cell_offsets(my, nu, nx, n2max, numax):
    """scenario_tables.h qr_tables: cells in the order N2 = 1 .. n2max, Nu = 1 .. min(N2, numax), each
    my min(N2, M) rows of width M + nx; -1 where there is no cell.  Returns (off [n2max numax], total)."""
    off = np.full(n2max * numax, -1, np.int32)
    total = 0
    for N2 in range(1, n2max + 1):
        for Nu in range(1, min(N2, numax) + 1):
            M = nu * Nu
            off[(N2 - 1) * numax + Nu - 1] = total
            total += my * min(N2, M) * (M + nx)
    return off, total


def mp_tables(case):
    """This cell's rows [my min(N2, M), M + nx] from mpmath, rounded to double: row my k + i = row k of
    [R_i | T_i]."""
    my, M, nx, N2, Nu = case["my"], case["M"], case["nx"], case["N2"], case["Nu"]
    rn = min(N2, M)
    cell = np.zeros((my * rn, M + nx))
    with mp.workdps(MP_DPS):
        for i in range(my):
            G = build_G(case["step"], case["n1"], i, N2, Nu)
            a = [[mp.mpf(float(x)) for x in G[r]] + [mp.mpf(float(x)) for x in case["phi"][i, r]] for r in range(N2)]
            a = mp_householder(a, rn)
            for k in range(rn):
                cell[my * k + i] = [float(x) for x in a[k]]
    return cell


def with_tables(case, cell=None, stage=None, hole=False):
    """The case with a table scenario: offsets by cell_offsets over n2max = N2, numax = Nu (this cell is the
    last one), this cell's rows `cell` (default: mp_tables).  hole: this cell's offset is -1 while the other
    cells exist.  stage: what the rows' own rounding adds to the column constant c (default u)."""
    c = dict(case)
    off, total = cell_offsets(c["my"], c["nu"], c["nx"], c["n2max"], c["numax"])
    q = np.zeros(total)
    o = int(off[(c["N2"] - 1) * c["numax"] + c["Nu"] - 1])
    assert o >= 0, "no cell for this horizon pair"
    cell = mp_tables(case) if cell is None else cell
    q[o:o + cell.size] = cell.reshape(-1)
    if hole:
        off = off.copy()
        off[(c["N2"] - 1) * c["numax"] + c["Nu"] - 1] = -1
    c.update(qrt=q, qoff=off, table_stage=U if stage is None else stage, key=case["key"])
    return c


def table_in_use(case, inst):
    if not INSTANCES[inst]["tables"] or case.get("qrt") is None:
        return False
    return int(case["qoff"][(case["N2"] - 1) * case["numax"] + case["Nu"] - 1]) >= 0


# ---------------------------------------------------------------------------------------------
# the float64 restatement
def restate(case, inst, drop_last_row=False, k0_bump=0, delta=None, n1=None):
    """The block algorithm of gpc_prologue<..> in float64, all columns at once (the device's passes
    recompute the same reflections).  Negative-control switches: drop_last_row (the last row of the padded
    last block is never streamed), k0_bump (a table block starts k0_bump levels too high), delta / n1
    (other weights / first steps than the case's)."""
    I = INSTANCES[inst]
    khb, my, M, nx, Nu, N2 = I["khb"], case["my"], case["M"], case["nx"], case["Nu"], case["N2"]
    delta = case["delta"] if delta is None else delta
    n1 = case["n1"] if n1 is None else n1
    sq, sl = weights(delta, case["wsq"]), weights(case["lam"], case["wsq"])
    tab = table_in_use(case, inst)
    if tab:
        o = int(case["qoff"][(N2 - 1) * case["numax"] + Nu - 1])
        P = my * min(N2, M)
        rows = case["qrt"][o:o + P * (M + nx)].reshape(P, M + nx) * sq[np.arange(P) % my, None]
    else:
        P = my * N2
        rows = np.concatenate([np.hstack([build_G(case["step"], n1, i, N2, Nu), case["phi"][i, :N2]]) * sq[i]
                               for i in range(my)])
    nblk = (P + khb - 1) // khb
    pad = np.zeros((nblk * khb, M + nx))
    pad[:P] = rows
    if drop_last_row:
        pad[P - 1] = 0.0
    Rm = np.zeros((M, M + nx))
    Rm[np.arange(M), np.arange(M)] = sl[np.arange(M) // Nu]
    nrefl = 0
    with np.errstate(all="ignore"):
        for blk in range(nblk):
            w = pad[blk * khb:(blk + 1) * khb].copy()
            k0 = (blk * khb) // my + k0_bump if tab else 0
            for k in range(k0, M):
                nrefl += 1
                wk = w[:, k].copy()
                sig = float(wk @ wk)
                if sig == 0.0:
                    continue
                x0 = Rm[k, k]
                n = math.sqrt(x0 * x0 + sig) if math.isfinite(x0 * x0 + sig) else math.nan
                xpn = x0 + n
                v0 = -sig / xpn
                beta = xpn / (n * sig)
                f = beta * (v0 * Rm[k] + wk @ w)
                Rm[k] = Rm[k] - f * v0
                Rm[k, k] = n
                w -= np.outer(wk, f)
        R, T = Rm[:, :M].copy(), Rm[:, M:].copy()
        ok = bool(np.all(np.diag(R) > 0.0))
        out = dict(ok=ok, R=R, nrefl=nrefl)
        if ok:
            Ru = np.triu(R)

            def solve(B):
                X = np.zeros_like(B)
                for kk in range(M - 1, -1, -1):
                    X[kk] = (B[kk] - Ru[kk, kk + 1:] @ X[kk + 1:]) / Ru[kk, kk]
                return X

            out.update(A=-solve(T), Rinv=solve(np.eye(M)))
    return out


def reflections(case, inst):
    """The number of reflections the instance applies to this case (zero blocks' columns included)."""
    I = INSTANCES[inst]
    khb, my, M = I["khb"], case["my"], case["M"]
    if table_in_use(case, inst):
        P = my * min(case["N2"], M)
        return sum(max(M - (blk * khb) // my, 0) for blk in range((P + khb - 1) // khb))
    return ((my * case["N2"] + khb - 1) // khb) * M


def g_of(case, inst):
    """g of the module docstring for this case and instance."""
    c = reflections(case, inst) * gamma_ref(INSTANCES[inst]["khb"]) + 6 * U
    if table_in_use(case, inst):
        c += case.get("table_stage", U)
    return 2 * c + c * c


def forward_bounds(case, inst, tr):
    """Column-wise bounds of |R^ - R|, |A^ - A*| and |Rinv^ - Rinv*| (2-norms of columns) from the truth:
    R: cond(W) g |R_:j|.  A (least squares, Higham Theorem 20.1 to first order with the relative
    perturbation g of W and V): cond g (|A*_:j| + (|V_:j| + cond res_j) / |W|_2).  Rinv: with R^ = (I + X) R,
    |X| <= cond g, R^-1 moves by -R^-1 X and the solve adds gamma_{M + 1} cond: |Rinv|_2 cond (g + gamma_{M+1})."""
    g, cond, M = g_of(case, inst), tr["cond"], case["M"]
    Rn = np.sqrt((np.triu(tr["R"].astype(float)) ** 2).sum(axis=0))
    An = np.sqrt((tr["A"].astype(float) ** 2).sum(axis=0))
    return dict(R=cond * g * Rn, A=cond * g * (An + (tr["vn"] + cond * tr["res"]) / tr["smax"]),
                Rinv=np.full(M, (1.0 / tr["smin"]) * cond * (g + gamma(M + 1))))


# ---------------------------------------------------------------------------------------------
# the LDS image
def sentinel_image(n):
    return np.full(n, SENTINEL, np.uint64).view(np.float64)


def acol_of(case):
    return np.arange(case["nx"]) if case.get("acol") is None else np.asarray(case["acol"])


def image_of(case, inst, res, ldsn=None, pack_shift=0, a_swap=None):
    """What the probe dumps when the prologue computes `res` (restate's result): (lds [ldsn], flags [64]).
    Negative-control switches: pack_shift (the packed index of one R^-1 entry is off by that much), a_swap
    (two state columns whose A columns change places: a column taken from the wrong pass)."""
    I = INSTANCES[inst]
    M, Nu, nx, astride = case["M"], case["Nu"], case["nx"], case["astride"]
    L = layout_of(inst, M, Nu, astride)
    lds = sentinel_image(L["total"] if ldsn is None else ldsn)
    lds[:M * M] = res["R"].reshape(-1)
    flags = np.full(64, 1 if res["ok"] else 0, np.int32)
    if not res["ok"]:
        return lds, flags
    if I["rinv"]:
        if not I["packed"]:
            lds[L["ri"]:L["ri"] + M * M] = 0.0
        for i in range(M):
            for k in range(i, M):
                e = rinv_idx(i, k, M, I["packed"])
                if pack_shift and (i, k) == (M // 2, M - 1):
                    e += pack_shift
                lds[L["ri"] + e] = res["Rinv"][i, k]
    A = res["A"]
    if a_swap:
        A = A.copy()
        A[:, list(a_swap)] = A[:, list(a_swap)[::-1]]
    ac = acol_of(case)
    for m in range(M):
        if I["first"] and m % Nu:
            continue
        row = m // Nu if I["first"] else m
        lds[L["a"] + row * astride + ac] = A[m]
    return lds, flags


def parse_image(case, inst, lds, flags):
    """The image taken apart and its layout checked: every word outside sR, sRi and the mapped sA entries
    holds the sentinel, every word inside was written, the flag is uniform.  Returns dict(ok, R, Rinv, A);
    A has the M rows (first-move instances: NaN in the rows they do not store)."""
    I = INSTANCES[inst]
    M, Nu, nx, astride = case["M"], case["Nu"], case["nx"], case["astride"]
    L = layout_of(inst, M, Nu, astride)
    tag = (case["key"], I["name"])
    flags = np.asarray(flags)
    assert flags.shape == (64,) and np.all(flags == flags[0]) and int(flags[0]) in (0, 1), tag + ("flag", flags.tolist())
    ok = bool(flags[0])
    bits = np.ascontiguousarray(lds, np.float64).view(np.uint64)
    assert bits.size >= L["total"], tag
    written = np.zeros(bits.size, bool)
    written[:M * M] = True
    ac = acol_of(case)
    assert len(set(ac.tolist())) == nx and ac.min() >= 0 and ac.max() < astride, tag
    nrow = M // Nu if I["first"] else M
    if ok:
        if I["rinv"]:
            written[L["ri"]:L["a"]] = True
        for r in range(nrow):
            written[L["a"] + r * astride + ac] = True
    keep = bits == np.uint64(SENTINEL)
    assert not np.any(keep & written), tag + ("not written", np.nonzero(keep & written)[0][:8].tolist())
    assert np.all(keep | written), tag + ("written outside", np.nonzero(~keep & ~written)[0][:8].tolist())
    v = np.asarray(lds, np.float64)
    out = dict(ok=ok, R=v[:M * M].reshape(M, M).copy())
    if not ok:
        return out
    if I["rinv"]:
        Ri = np.zeros((M, M))
        for i in range(M):
            for k in range(i, M):
                Ri[i, k] = v[L["ri"] + rinv_idx(i, k, M, I["packed"])]
        if not I["packed"]:
            full = v[L["ri"]:L["a"]].reshape(M, M)
            low = full[np.tril_indices(M, -1)]
            assert np.all(low == 0.0) and not np.any(np.signbit(low)), tag + ("R^-1 below the diagonal",)
        out["Rinv"] = Ri
    A = np.full((M, nx), np.nan)
    for r in range(nrow):
        A[r * Nu if I["first"] else r] = v[L["a"] + r * astride + ac]
    out["A"] = A
    return out


# ---------------------------------------------------------------------------------------------
# the check of one case
def measure(case, inst, got, tr):
    """The ratios of what `got` (parse_image's or restate's dict) shows to every bound: rr, ra, ri the three
    invariants, fr, fa, fi the forward errors of R, A, Rinv over forward_bounds."""
    I = INSTANCES[inst]
    M, g = case["M"], g_of(case, inst)
    tiny = LD(1e-300)
    R = np.triu(np.asarray(got["R"], LD))
    out = {}
    wn, vn = np.asarray(tr["wn"], LD), np.asarray(tr["vn"], LD)
    WtW = tr["R"].T @ tr["R"]
    out["rr"] = float((np.abs(R.T @ R - WtW) / np.maximum(g * np.outer(wn, wn), tiny)).max())
    fb = forward_bounds(case, inst, tr)
    col = lambda D: np.sqrt((np.asarray(D, LD) ** 2).sum(axis=0)).astype(float)
    out["fr"] = float((col(R - np.triu(tr["R"])) / np.maximum(fb["R"], 1e-300)).max())
    A = np.asarray(got["A"], LD)
    rows = [m for m in range(M) if not (I["first"] and m % case["Nu"])]
    if not I["first"]:
        WtV = tr["R"].T @ tr["T"]
        bound = g * (np.outer(wn, vn) + np.abs(R.T) @ (np.abs(R) @ np.abs(A)))
        res = np.abs(R.T @ (R @ A) + WtV)
        out["ra"] = float(np.where(res == 0, LD(0), res / np.maximum(bound, tiny)).max())
    out["fa"] = float((col(A[rows] - tr["A"][rows]) / np.maximum(fb["A"], 1e-300)).max())
    if I["rinv"]:
        Ri = np.triu(np.asarray(got["Rinv"], LD))
        res = np.abs(R @ Ri - np.eye(M, dtype=LD))
        out["ri"] = float((res / np.maximum(LD(gamma(M + 1)) * (np.abs(R) @ np.abs(Ri)), tiny)).max())
        out["fi"] = float((col(Ri - tr["Rinv"]) / np.maximum(fb["Rinv"], 1e-300)).max())
    return out


@functools.lru_cache(maxsize=None)
def _restated_ratios(key, inst):
    case = CASES[key]
    return measure(case, inst, restate(case, inst), truth_of(case))


def check_case(case, inst, lds, flags, ratios=None):
    """Everything asserted about one case's dump.  Returns the ratios to the bounds (each asserted <= 1);
    with `ratios` (a dict) keeps the largest per name.  The forward errors of A and Rinv are held to
    8 x the larger of the restatement's own and the derived bound (fa, fi are then divided by that), and are
    left out, as the issue sets it, in the stiff family (case["stiff"])."""
    I = INSTANCES[inst]
    tag = (case["key"], I["name"])
    got = parse_image(case, inst, lds, flags)
    assert got["ok"] == case.get("expect_ok", True), tag + ("flag", got["ok"])
    if not got["ok"]:
        return {}
    tr = truth_of(case)
    M = case["M"]
    R = got["R"]
    assert np.all(np.isfinite(R[np.triu_indices(M)])) and np.all(np.diag(R) > 0.0), tag + ("R",)
    assert np.all(np.isfinite(got["A"][~np.isnan(got["A"]).all(axis=1)])), tag + ("A",)
    if I["rinv"]:
        assert np.all(np.isfinite(got["Rinv"])), tag + ("Rinv",)
    out = measure(case, inst, got, tr)
    ref = _restated_ratios(case["key"], inst) if case["key"] in CASES and CASES[case["key"]] is case else \
        measure(case, inst, restate(case, inst), tr)
    for k in ("fa", "fi"):
        if k in out:
            if case.get("stiff"):
                del out[k]
            else:
                out[k] /= 8.0 * max(ref[k], 1.0)
    for k, v in out.items():
        assert v <= 1.0, tag + (k, v, "cond %.3g g %.3g" % (tr["cond"], g_of(case, inst)))
        if ratios is not None:
            ratios[k] = max(ratios.get(k, 0.0), v)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---------------------------------------------------------------------------------------------
# the probe's arguments
def pack_launch(inst, cases):
    """(hdr, dpool, ipool) of one launch: every case's arrays appended to the two pools."""
    dp, ip, hdr = [], [], []
    nd = ni = 0

    def put_d(a):
        nonlocal nd
        a = np.ascontiguousarray(a, np.float64).reshape(-1)
        dp.append(a)
        nd += a.size
        return nd - a.size

    def put_i(a):
        nonlocal ni
        a = np.ascontiguousarray(a, np.int32).reshape(-1)
        ip.append(a)
        ni += a.size
        return ni - a.size

    for c in cases:
        h = dict(inst=inst, my=c["my"], nu=c["nu"], nx=c["nx"], wsq=c["wsq"], tlen=c["step"].shape[2],
                 n2max=c["n2max"], numax=c["numax"], M=c["M"], Nu=c["Nu"], N2=c["N2"], astride=c["astride"],
                 step_off=put_d(c["step"]), phi_off=put_d(c["phi"]), n1_off=put_i(c["n1"]),
                 delta_off=put_d(c["delta"]), lambda_off=put_d(c["lam"]),
                 acol_off=-1 if c.get("acol") is None else put_i(c["acol"]), qrt_off=-1, qrt_len=0, qoff_off=-1)
        if c.get("qrt") is not None:
            h.update(qrt_off=put_d(c["qrt"]), qrt_len=c["qrt"].size, qoff_off=put_i(c["qoff"]))
        hdr.append([h[k] for k in HDR])
    return np.array(hdr, np.int32), np.concatenate(dp), np.concatenate(ip)


# ---------------------------------------------------------------------------------------------
# the seeded cases
N1_CYCLE = (0, 1, 3)
# (family, index) whose default seed cannot keep cond(W) <= COND_CAP get another seed here; none is skipped
CASE_SEED = {}


def make_case(key, my, nu, Nu, N2, nx, seed, wsq=0, astride=None, acol=False, dead=(), zero_in=None,
              lam_zero=None, nan_delta=None, pole=(0.3, 0.8), lam_scale=None, n2max=None, numax=None):
    """One synthetic case.  Step responses s_in(t) = gain (1 - p^(t + 1 - d)) from t = d on (d the entry's
    dead time, 0..2; `dead`: inputs with d = 40 for every output, so their columns of G are exactly zero over
    the horizon; zero_in: an input whose step response is identically zero), phi standard normal, n1 cycling
    0, 1, 3, weights log-uniform over 1e-5 .. 1 (their squares, with wsq) with random signs."""
    rng = np.random.default_rng(41000 + seed)
    M = nu * Nu
    n2max = N2 if n2max is None else n2max
    numax = Nu if numax is None else numax
    n1 = np.array([N1_CYCLE[i % 3] for i in range(my)], np.int32)
    tlen = int(n1.max()) + n2max + 1
    step = np.zeros((my, nu, tlen))
    t = np.arange(tlen)
    for i in range(my):
        for n in range(nu):
            d = 40 if n in dead else int(rng.integers(0, 3))
            gain = rng.uniform(0.3, 1.5) * rng.choice([-1.0, 1.0])
            p = rng.uniform(*pole)
            step[i, n] = np.where(t >= d, gain * (1.0 - p ** np.maximum(t + 1 - d, 0)), 0.0)
    if zero_in is not None:
        step[:, zero_in] = 0.0
    phi = rng.standard_normal((my, n2max, nx))
    lo = -2.5 if wsq else -5.0
    delta = 10.0 ** rng.uniform(lo, 0.0, my) * rng.choice([-1.0, 1.0], my)
    lam = 10.0 ** rng.uniform(lo, 0.0, nu) * rng.choice([-1.0, 1.0], nu)
    delta[0], lam[0] = (1.0, -(10.0 ** lo))          # both ends of the span in every case
    if lam_scale is not None:
        lam = lam * lam_scale
    if lam_zero is not None:
        lam[lam_zero] = 0.0
    if nan_delta is not None:
        delta[nan_delta] = math.nan
    ac = None
    if acol:
        astride = 36 if astride is None else astride      # kSmA, the small kernel's row stride
        ac = rng.permutation(astride)[:nx].astype(np.int32)
    return dict(key=key, my=my, nu=nu, Nu=Nu, N2=N2, M=M, nx=nx, wsq=wsq, n2max=n2max, numax=numax, n1=n1,
                step=step, phi=phi, delta=delta, lam=lam, astride=nx if astride is None else astride, acol=ac,
                expect_ok=lam_zero is None and nan_delta is None)


def stiff_case(key, seed, **kw):
    """A slow plant (poles 0.95 .. 0.98) with fewer rows of G than moves (my N2 < M) whose lambda is scaled, by bisection on the float64 singular values,
    until cond(W) lies just below COND_CAP: 5e5 .. 1e6 (asserted from the truth on the CPU)."""
    lo, hi = -12.0, 0.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        c = make_case(key, seed=seed, pole=(0.95, 0.98), lam_scale=10.0 ** mid, **kw)
        W, _ = build_W(c["step"], c["phi"], c["n1"], c["delta"], c["lam"], c["wsq"], c["N2"], c["Nu"])
        s = np.linalg.svd(W, compute_uv=False)
        if s[0] / s[-1] > 0.75 * COND_CAP:
            lo = mid
        else:
            hi = mid
    c = make_case(key, seed=seed, pole=(0.95, 0.98), lam_scale=10.0 ** hi, **kw)
    c["stiff"] = True
    return c


def derived(case, key, **changes):
    c = dict(case)
    c.update(changes)
    c["key"] = key
    return c


def _families():
    F, C = {}, {}

    def fam(name, insts, cases, pairs=()):
        for c in cases:
            assert c["key"] not in C, c["key"]
            C[c["key"]] = c
        F[name] = dict(insts=tuple(insts), keys=[c["key"] for c in cases], pairs=tuple(pairs))

    def mk(name, idx, *a, **kw):
        key = "%s/%d" % (name, idx)
        return make_case(key, *a, seed=CASE_SEED.get((name, idx), 100 * len(F) + idx), **kw)

    # (my, nu, Nu, N2, nx).  MAXM 16, streamed: M = 1; M = MAXM with my N2 a multiple of 8 and of 12; 15 and
    # 23 rows (one short of a block); 6 rows (less than a block, N2 < M); Nu = M with N2 < M; my = 5, N2 < M
    n = "stream16"
    fam(n, (0, 4, 9), [mk(n, 0, 1, 1, 1, 1, 3), mk(n, 1, 3, 2, 8, 8, 5, astride=7), mk(n, 2, 3, 3, 5, 5, 7, wsq=1),
                       mk(n, 3, 1, 2, 3, 23, 4), mk(n, 4, 2, 2, 2, 3, 5), mk(n, 5, 1, 1, 7, 2, 3, wsq=1),
                       mk(n, 6, 5, 3, 4, 3, 6, dead=(1,))])
    # passes at MAXM 16, M = 16 (vper = 48): M + nx = 63, 64, 65 and 113 (three passes), one W; the A columns
    # of the two-pass case again with permuted Phi columns and with single columns of pass 0 and pass 1
    n = "pass16"
    b = mk(n, 0, 2, 2, 8, 9, 113)
    perm = np.random.default_rng(7).permutation(49)
    ps = [derived(b, "%s/nx%d" % (n, nx), nx=nx, astride=nx, phi=b["phi"][:, :, :nx].copy()) for nx in (47, 48, 49)]
    ps.append(derived(b, n + "/perm", nx=49, astride=49, phi=b["phi"][:, :, perm].copy(), perm=perm))
    ps += [derived(b, "%s/col%d" % (n, j), nx=1, astride=1, phi=b["phi"][:, :, j:j + 1].copy(), col=j) for j in (0, 47, 48)]
    fam(n, (0,), [b] + ps)
    # MAXM 32: M = MAXM in one (nx 32) and two passes (nx 33) and three (nx 65), M = 17 with Nu = M
    n = "stream32"
    b = mk(n, 0, 2, 4, 8, 10, 65)
    fam(n, (1,), [b] + [derived(b, "%s/nx%d" % (n, nx), nx=nx, astride=nx, phi=b["phi"][:, :, :nx].copy()) for nx in (31, 32, 33)]
        + [mk(n, 1, 2, 1, 17, 20, 5, astride=6)])
    # MAXM 64: M = 63 (vper = 1) with nx = 1 .. 4 (one to four passes), M = 33 at M + nx = 63, 64, 65
    n = "stream64"
    b = mk(n, 0, 3, 7, 9, 32, 4)
    b2 = mk(n, 1, 2, 3, 11, 12, 32, wsq=1)
    fam(n, (2,), [b] + [derived(b, "%s/nx%d" % (n, nx), nx=nx, astride=nx, phi=b["phi"][:, :, :nx].copy()) for nx in (1, 2, 3)]
        + [b2] + [derived(b2, "%s/b_nx%d" % (n, nx), nx=nx, astride=nx, phi=b2["phi"][:, :, :nx].copy()) for nx in (30, 31)])
    # the table path, kHB = 12, acol into 36 columns: my = 1, 2, 3, 5 (5 and, below N2 = 4, 3 do not divide
    # 12: blocks straddle levels), N2 < M, M = 1, one exact block (12 rows), Shell's shape (45 rows, nx 35)
    n = "tables"
    fam(n, (3, 4, 9), [with_tables(c) for c in (
        mk(n, 0, 1, 2, 3, 9, 5, acol=True), mk(n, 1, 2, 3, 5, 15, 7, acol=True), mk(n, 2, 3, 3, 5, 30, 35, acol=True),
        mk(n, 3, 5, 2, 8, 10, 6, acol=True, wsq=1), mk(n, 4, 5, 1, 1, 1, 2, acol=True),
        mk(n, 5, 3, 3, 4, 4, 6, acol=True, dead=(2,)), mk(n, 6, 5, 2, 5, 7, 9, acol=True))])
    # first-move rows, kHB = 4: 9, 16 (a multiple of 4), 7 (one short) rows at MAXM 16; 30 and 11 rows at 32
    n = "first16"
    fam(n, (5, 7), [mk(n, 0, 1, 1, 5, 9, 6), mk(n, 1, 2, 2, 8, 8, 5, astride=8), mk(n, 2, 1, 3, 3, 7, 4, wsq=1),
                    mk(n, 3, 1, 1, 1, 1, 2)])
    n = "first32"
    fam(n, (6, 8), [mk(n, 0, 2, 2, 12, 15, 9), mk(n, 1, 1, 4, 8, 11, 5, astride=6)])
    # not positive definite: lambda = 0 on an input whose step response is identically zero; a NaN weight
    n = "notpd"
    fam(n, (0, 3, 5), [mk(n, 0, 2, 2, 3, 6, 4, zero_in=1, lam_zero=1, acol=True),
                       mk(n, 1, 2, 2, 3, 6, 4, nan_delta=1, acol=True)])
    # the stiff family: cond(W) just below 1e6
    n = "stiff"
    fam(n, (0, 3), [with_tables(stiff_case("%s/%d" % (n, k), 900 + k, my=m, nu=u, Nu=v, N2=h, nx=4, acol=True))
                    for k, (m, u, v, h) in enumerate(((1, 2, 6, 8), (2, 3, 4, 4)))])
    return F, C


FAMILIES, CASES = _families()


def family_cases(name, inst):
    """The cases of one launch.  A TABLES = false instance never reads the tables; they stay in the case."""
    return [CASES[k] for k in FAMILIES[name]["keys"]]
