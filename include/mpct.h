/*
 * mpct.h — C ABI of the MI355X batched closed-loop GPC scoring engine (libmpct.so).
 *
 * Drop-in boundary for the reference's per-candidate closed-loop seam
 *   function [y,u,t,ys,uopt] = closedloop_toolbox(mpc_toolbox,r,v,N,Nu,delta,lambda,nit)
 *   (MPC-Tuning/MPC_Tuning/closedloop_toolbox.m:1), called once per candidate (and once per
 *   output for square plants) by VNS2.m:153,168 and GAM_fun.m:81.
 * Here one call scores a whole BATCH of candidates (N2, Nu, delta, lambda) on the GPU.  A
 * MATLAB host binds it with loadlibrary('libmpct','mpct.h') / calllib, or through the MEX
 * shim in INTEGRATION.md; the Python host mirror (mpct/) binds it with ctypes.
 *
 * Conventions
 *   - plain C types only; every matrix is row-major double; "row signals" are [row][t].
 *   - the caller owns every input/output buffer; the library owns the scenario (host tables
 *     and their device copies) until mpct_scenario_destroy.
 *   - negative return codes are argument / shape / device errors (message in
 *     mpct_last_error(), thread-local); per-candidate numerical trouble never fails the call:
 *     it is reported in mpct_result.status[] with NaN costs (the reference swallows such
 *     errors with fprintf and continues: VNS2.m:161-163, GAM_fun.m:82-84).
 *   - threading: one scenario per host thread, or external synchronisation.  All device work
 *     of a call is complete when mpct_eval_batch returns.  A scenario keeps one context per GPU
 *     it has been evaluated on (table copies, sort buffers, a library-owned stream); the
 *     host-pointer entries synchronise that stream only, never the whole device.
 *   - robust scoring (mpct_robust_result, mpct_eval_robust, mpct_eval_robust_device,
 *     mpct_robust_instance) is part of ABI 7: new exports and one new struct, added without a
 *     version change because no existing struct, export or behaviour changes.  The tail statistics
 *     (mpct_robust_tail, mpct_eval_robust_tail, mpct_eval_robust_tail_device) were added the same way,
 *     and so was the Pareto analysis of a scored grid (mpct_pareto_result, mpct_pareto_device, mpct_pareto),
 *     and the closed-loop performance indices (mpct_index_params, mpct_index_result, mpct_indices_device,
 *     mpct_indices, mpct_eval_indices, mpct_eval_indices_device), and the statistics of any per-simulation
 *     table over its draws (mpct_draw_stats_result, mpct_draw_stats_device, mpct_draw_stats,
 *     mpct_eval_robust_indices, mpct_eval_robust_indices_device), and the hypervolume of a front with its
 *     members' exclusive contributions (mpct_hv_result, mpct_hypervolume_device, mpct_hypervolume), and
 *     the greedy selection of the members that carry a front (mpct_hv_select_result,
 *     mpct_hv_select_device, mpct_hv_select), and the exact hypervolume and contributions for up to three
 *     objectives (mpct_hvx_result, mpct_hypervolume_exact_device, mpct_hypervolume_exact), and the limit
 *     indices (mpct_limit_params, mpct_limit_result, mpct_limit_indices_device, mpct_limit_indices,
 *     mpct_eval_limit_indices, mpct_eval_limit_indices_device, mpct_eval_robust_limit_indices,
 *     mpct_eval_robust_limit_indices_device), and the step-response indices per setpoint segment
 *     (mpct_segment_params, mpct_segment_result, mpct_reference_segments, mpct_segment_indices_device,
 *     mpct_segment_indices, mpct_eval_segment_indices, mpct_eval_segment_indices_device,
 *     mpct_eval_robust_segment_indices, mpct_eval_robust_segment_indices_device), and the oscillation
 *     indices per setpoint segment (mpct_osc_params, mpct_osc_result, mpct_osc_indices_device,
 *     mpct_osc_indices, mpct_eval_osc_indices, mpct_eval_osc_indices_device, mpct_eval_robust_osc_indices,
 *     mpct_eval_robust_osc_indices_device), and the goal-attainment selection (mpct_goal_result,
 *     mpct_goal_attain_device, mpct_goal_attain), and the trajectory envelopes over the plant draws
 *     (mpct_envelope_spread, mpct_envelope_device, mpct_envelope, mpct_eval_robust_envelope,
 *     mpct_eval_robust_envelope_device).
 */
#ifndef MPCT_H
#define MPCT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPCT_ABI_VERSION 7 /* 7: every simulation slot is prefilled with MPCT_ST_NOT_RUN and NaN costs
                              before the class launches (a slot no launch simulates stays so).
                              6: strided multi-device shards (mpct_shard_candidates replaces the
                              contiguous mpct_shard_range), a device may appear more than once in
                              mpct_eval_batch_multi's list; dims table carries nit, nq.
                              5: one scenario on several GPUs of one process (mpct_eval_batch_multi),
                              kernel-instance query; the host-pointer entries wait on
                              their own stream only.  4: nonlinear MPC scenarios (mpct_nmpc_scenario_create); 3: MD feed-forward +
                              soft output bands; 2: DTC-GPC predictor + plant-only disturbances + plant
                              variants; v1..v3 descriptors accepted */

/* error codes */
#define MPCT_OK 0
#define MPCT_EINVAL (-1)   /* bad argument / shape                                  */
#define MPCT_ENOMEM (-2)   /* host or device allocation failed                      */
#define MPCT_EDEVICE (-3)  /* HIP runtime error (no device, launch failure, ...)    */
#define MPCT_ERANGE (-4)   /* a size exceeds what the compiled kernels support       */

/* per-simulation status bits (mpct_result.status) */
#define MPCT_ST_OK 0
#define MPCT_ST_QP_MAXITER 1   /* active-set iteration cap hit at some step          */
#define MPCT_ST_QP_INFEAS 2    /* QP infeasible at some step (dual unbounded)        */
#define MPCT_ST_NONFINITE 4    /* a non-finite value appeared in the state           */
#define MPCT_ST_SKIPPED 8      /* padding / sentinel candidate (N2 <= 0)             */
#define MPCT_ST_BADHORIZON 16  /* N2/Nu outside the scenario's range or Nu > N2      */
#define MPCT_ST_SQP_MAXITER 32 /* NMPC: a Gauss-Newton SQP hit sqp_max at some step  */
#define MPCT_ST_BOUNDS 64      /* NMPC: the closed loop left the state/OV bounds     */
#define MPCT_ST_NOT_RUN 128    /* no kernel launch simulated this slot (an internal
                                  dispatch fault; costs NaN).  Every slot is prefilled
                                  with it before the class launches, which overwrite it */

/* One SISO discrete transfer function  y = z^-delay * num(z)/den(z) u  in the form tfdata(.,'v')
 * returns it (descending powers of z, numerator padded to the denominator's length, den[0]=1)
 * — the representation descompMPC.m:19 reads.  len = number of coefficients of each. */
typedef struct mpct_dtf {
  int32_t len;
  const double* num;
  const double* den;
  int32_t delay;
} mpct_dtf;

/* Scenario: everything that does not depend on the candidate.
 *   plant[i*(nu+nd)+j]  : simulated plant entries (the toolbox's sim simulates the model
 *                         itself unless options.Model is set: closedloop_toolbox.m:50)
 *   model[i*(nu+nd)+j]  : prediction model entries, used for the MatG step responses
 *                         (MatG.m:51 step(Ps(i,j),...))
 *   carima_A / carima_B : the CARIMA form after descompMPC + BA_MIMO (DTC_GPC_WW.m:79):
 *                         A_i (na[i]+1 coeffs, z^-1 powers, A_i[0]=1) concatenated over i;
 *                         B_ij (nb[i*(nu+nd)+j]+1 coeffs) concatenated row-major over (i,j);
 *                         dp[i*(nu+nd)+j] the descompMPC delays.  abi >= 5, dtc == 0, mdband == 0:
 *                         na, carima_A, nb, carima_B and dp may ALL be NULL; the library then
 *                         derives them from `model` (descompMPC.m:19-43, then the exact LCM of
 *                         each row's distinct denominators: the toolbox-equivalent CARIMA form).
 *   n1[i]               : first predicted step of output i: 1 = toolbox window t+1..t+N2
 *                         (PredictionHorizon semantics), dmin_i+1 = GPC window (MatG.m:64,
 *                         diophantine.m:44 N1 = d+1)
 *   weights_squared     : 1 = toolbox cost (Weights enter squared), 0 = DTC_GPC_WW.m:67-76
 *   du_min..u_max[nu]   : MV rate / amplitude bounds (already scaled, MPCTuning.m:170-178);
 *                         +-INFINITY disables a bound
 *   n2_max, nu_max      : largest horizons any candidate of this scenario may use
 *   nit                 : closed-loop length (Par.nit);  vns_ink: VNS2.m:43 inK (1-based)
 *   yref[my*nit]        : GAM/VNS reference trajectory Par.Yref (MPCTuning.m:188,320)      */
typedef struct mpct_scenario_desc {
  int32_t abi_version; /* = MPCT_ABI_VERSION */
  int32_t my, nu, nd;
  int32_t nit;
  int32_t n2_max, nu_max;
  int32_t weights_squared;
  int32_t vns_ink;
  const int32_t* n1;
  const mpct_dtf* plant;
  const mpct_dtf* model;
  const int32_t* na;
  const double* carima_A;
  const int32_t* nb;
  const double* carima_B;
  const int32_t* dp;
  const double* du_min;
  const double* du_max;
  const double* u_min;
  const double* u_max;
  const double* yref;
  /* ---- abi_version >= 2 (ignored for version 1 descriptors) -------------------------------
   * dtc      1: DTC-GPC (DTC_GPC_WW.m:126-164): the free response is driven by the predictor
   *             yp = Gz*u + Fr*(y - Pz*u) (OptimalPredictor2.m:24-40) instead of the measured y.
   *             The caller passes the model with its real delays (MatG window n1 = dmin+1),
   *             dp = dnz = descompMPC delays minus dmin (deltaUFree.m / DTC_GPC_WW.m:91-93) and
   *             the Diophantine window starts at d = 0 (DTC_GPC_WW.m:80).  Requires open_loop 0.
   * filter   [my] Fr_i(z) (mimofilter.m / filtro_siso.m), delay 0; NULL -> Fr = 1
   * nq       plant-only disturbance inputs: they drive the simulated plant through dist and are
   *             never seen by the controller's model (DTC_GPC_WW.m:29-30 Pq, :128-129)
   * dist     [my*nq] disturbance paths; their signals are the rows of eval's v: [nref][nd+nq][nit] */
  int32_t dtc;
  const mpct_dtf* filter;
  int32_t nq;
  const mpct_dtf* dist;
  /* nplant     number of simulated-plant variants (plant-mismatch Monte-Carlo draws, SURVEY
   *            §8d config 4); 0 or 1 -> the single plant above.  Simulation s = c*nref + k runs
   *            variant k % nplant (the draws ride on the reference dimension).  Variants do not
   *            change which kernel runs: a GPC-mode scenario stays on gpc_small_kernel (cost-only
   *            batches) when every entry of EVERY variant is within its limits (<= 4 plant terms,
   *            taps within the input ring), e.g. the Shell 3x3 model-error draws of
   *            Shell3x3.m:34-48; one variant outside them and the general kernel runs all
   * plant_var  [nplant][my*(nu+nd)] variant plants (replace plant when nplant > 1)           */
  int32_t nplant;
  const mpct_dtf* plant_var;
  /* ---- abi_version >= 3 --------------------------------------------------------------------
   * mdband   1: the toolbox MPC with measured-disturbance feed-forward and soft output bands
   *             (Shell7x5.m:112-196, WoodBerry.m:102-148; mdband_kernel.hip).  MD
   *             columns nu..nu+nd-1 of plant/model enter the prediction held at v(t)
   *             (mpcsimopt MDLookAhead 'off'); OV Min/Max are softened by MinECR/MaxECR with ONE
   *             slack eps >= 0 weighted by rho_ecr (Weights.ECR); Weights.OV / Weights.MVRate act
   *             over the ScaleFactors.  mpct_scenario_create requires plant == model
   *             (closedloop_toolbox.m:50 sims the model) and nplant <= 1; mpct_scenario_create_est with
   *             MPCT_EST_OUTPUT_BIAS lifts both.  Requires n1[i] == 1 (PredictionHorizon window), dtc == 0, nq == 0 and
   *             nu*nu_max + 1 <= 64.  na/carima_A/nb/carima_B/dp may be NULL (no Diophantine tables).
   * y_min, y_max [my]      OV Min / Max, already scaled (MPCTuning.m:180-181); +-INFINITY: none
   * ecr_min, ecr_max [my]  OV MinECR / MaxECR (0: hard output bound)
   * y_scale [my], u_scale [nu]  OV / MV ScaleFactor after MPCTuning.m:175-184 (NULL: all 1)
   * rho_ecr                Weights.ECR (Shell7x5.m:191, MPCTuning.m:354)                       */
  int32_t mdband;
  const double* y_min;
  const double* y_max;
  const double* ecr_min;
  const double* ecr_max;
  const double* y_scale;
  const double* u_scale;
  double rho_ecr;
} mpct_scenario_desc;

typedef struct mpct_scenario mpct_scenario;

/* Nonlinear MPC scenario (config 5): the seam
 *   function [y,u,yopt,uopt] = closedloop_toolbox_nmpc(nmpcobj,model,init,r,N,Nu,delta,lambda,nit)
 *   (Matlab-Toolbox/NMPC/closedloop_toolbox_nmpc.m:1; callers VNS2.m:155, GAM_fun.m:87,
 *   MPC-Tuning/VanDeVusse_NMPC.m:244).  MATLAB passes the model as a function handle; a C ABI
 *   cannot carry one to the GPU, so the model is chosen from the library's built-in families by id
 *   with its parameters:
 *     model  MPCT_NMPC_VANDEVUSSE: nmpc_vandevusse_state.m (nx = 3, nu = 2), params[16] in the
 *            order of nmpc_vandevusse_state.m:43-58 (k10 k20 k30 E1 E2 E3 dHab dHbc dHad rho cp
 *            Kw Ar V T0 Ca0); NULL = the reference's values
 *   xc[ny]          output states, 1-based as init.xc (VanDeVusse_NMPC.m:82: [2 3]); ny <= 2
 *   ts, nsub        Ts and the fixed RK4 sub-steps per Ts that replace ode15s / the toolbox's
 *                   discretisation (plant and prediction use the same integrator)
 *   x0[nx], u0[nu]  init.x0, init.u0
 *   u_min/u_max[nu] MV Min/Max (hard); x_min/x_max[nx] hard state bounds, linearised in
 *                   every SQP subproblem (+-inf = none; a closed loop whose states still leave
 *                   them is flagged MPCT_ST_BOUNDS); y_scale[ny], u_scale[nu] OV / MV ScaleFactor
 *   n_max, nu_max   largest prediction / control horizon any candidate uses (nu*nu_max <= 32)
 *   nit, yref[ny*nit], vns_ink  as in mpct_scenario_desc
 *   sqp_max, sqp_tol  Gauss-Newton iteration cap per controller call and the stopping test
 *                   max |change of an absolute move| / u_scale <= sqp_tol (0: 100 and 1e-8); each
 *                   step is globalised by Armijo backtracking on the cost
 * Evaluate with mpct_eval_batch(_device) exactly like a linear scenario: N2[] holds N, delta[] the
 * OV weights, lambda[] the MVRate weights, r[] the reference sets (ny rows), v = NULL; ys / uopt
 * are yopt / uopt; qp_iters counts Gauss-Newton iterations. */
#define MPCT_NMPC_VANDEVUSSE 1
typedef struct mpct_nmpc_desc {
  int32_t abi_version; /* >= 4 */
  int32_t model;
  int32_t nx, ny, nu;
  const double* params;
  const int32_t* xc;
  double ts;
  int32_t nsub;
  const double* x0;
  const double* u0;
  const double* u_min;
  const double* u_max;
  const double* x_min;
  const double* x_max;
  const double* y_scale;
  const double* u_scale;
  int32_t n_max, nu_max;
  int32_t nit;
  const double* yref;
  int32_t vns_ink;
  int32_t sqp_max;
  double sqp_tol;
} mpct_nmpc_desc;

/* Build a nonlinear MPC scenario (no device needed).  Returns MPCT_OK. */
int32_t mpct_nmpc_scenario_create(const mpct_nmpc_desc* desc, mpct_scenario** out);

/* The same scenario with a simulated plant that is not the controller's model (an addition to ABI 7:
 * no struct, export or behaviour changes).  The reference's seam keeps the two apart: `model` is the
 * plant handle integrated at closedloop_toolbox_nmpc.m:71 and :91, the controller predicts with
 * nmpcobj.Model.StateFcn and is fed the measured plant state (:69): full state feedback, no estimator,
 * so a steady-state offset under mismatch is part of the result.
 *   nplant = 0      exactly mpct_nmpc_scenario_create; plant_params and plant_x0 must be NULL
 *   nplant >= 1     simulation s = c*nref + k runs plant variant k % nplant (the convention of
 *                   mpct_scenario_desc.nplant / plant_var)
 *   plant_params    [nplant][16], each row in the order of desc->params
 *   plant_x0        [nplant][nx] start state of each variant, or NULL: every variant starts at desc->x0
 * The controller keeps desc->params for the prediction, its tangents, the Armijo trials and the
 * linearised state rows.  Variant k's parameters integrate the closed-loop plant step from variant k's
 * x0, and the plant of the open-loop leg (ys) too; the open-loop controller call starts from the
 * variant's x0.  open_loop and want_traj stay legal.  A draw whose states leave x_min / x_max comes
 * back with MPCT_ST_BOUNDS: a result, not an error (mpct_eval_robust counts it as a failed draw).
 * MPCT_EINVAL: nplant < 0; nplant = 0 with a non-NULL table; nplant >= 1 with plant_params NULL; a
 * non-finite parameter or start state; a variant with rho*cp*V = 0. */
int32_t mpct_nmpc_scenario_create_var(const mpct_nmpc_desc* desc, int32_t nplant, const double* plant_params,
                                      const double* plant_x0, mpct_scenario** out);

/* Evaluation options. */
typedef struct mpct_opts {
  int32_t open_loop;   /* 1: also compute the open-loop first-move prediction (uopt, ys) and
                          the VNS terms j21/Jnu (closedloop_toolbox.m:85-100); 0: closed loop
                          + J1/j22 only (all GAM_fun needs, GAM_fun.m:81)                  */
  int32_t want_traj;   /* 1: write y/u (and ys/uopt if open_loop) trajectories             */
  int32_t max_qp_iter; /* active-set iteration cap per step (0 = default 8*M)              */
  int32_t device;      /* HIP device ordinal (-1 = current)                               */
  double feas_tol;     /* constraint feasibility tolerance (0 = default 1e-10)            */
} mpct_opts;

/* Results, one row per SIMULATION s = c*nref + k (candidate c, reference k).  Any pointer may
 * be NULL to skip that output.  Sizes: J1/j21/j22 [S*my], Jnu [S*nu], status/qp_iters [S],
 * y/ys [S*my*nit], u/uopt [S*nu*nit].
 *   J1[i]  = sum_t (y_i - yref_i)^2                       GAM_fun.m:110-111
 *   j21[i] = sum_{t>=inK} (y_i - ys_i)^2                   VNS2.m:172,176
 *   j22[i] = sum_{t>=inK} (y_i - yref_i)^2                 VNS2.m:173,177
 *   Jnu[n] = sum_t (|uopt_n(1)| / |diff(uopt_n)|)^2, inf/NaN -> 0   VNS2.m:183-191
 * Only the requested arrays are written, and only their S rows.  In a call without open_loop, j21 and
 * Jnu (when requested) come back NaN.  All ten pointers NULL is legal: the batch is checked and
 * simulated, nothing is written, and the call returns MPCT_OK (the robust entries reject an `out`
 * without a pointer instead; they have nothing else to deliver).  A simulation whose status carries
 * MPCT_ST_SKIPPED or MPCT_ST_BADHORIZON is not run: like its costs, its rows of the trajectories the
 * call writes (y, u; ys, uopt with open_loop) come back NaN, through every entry.                   */
typedef struct mpct_result {
  double* J1;
  double* j21;
  double* j22;
  double* Jnu;
  int32_t* status;
  int64_t* qp_iters;
  double* y;
  double* u;
  double* ys;
  double* uopt;
} mpct_result;

/* Version / capability query (no device needed). */
int32_t mpct_abi_version(void);
const char* mpct_last_error(void);

/* Build a scenario: validates the description, precomputes the candidate-independent tables on
 * the host (step responses s_ij(t), Diophantine F rows, deltaUFree/cell2mat2 past-control
 * rows; see DESIGN.md §Data layout).  Does NOT touch the GPU (device copies are made on first
 * evaluation), so it is usable on a CPU-only host for inspection.  Returns MPCT_OK. */
int32_t mpct_scenario_create(const mpct_scenario_desc* desc, mpct_scenario** out);

/* Build a band-kernel scenario whose simulated plant differs from the controller's model (an
 * addition to ABI 7: no struct, export or behaviour of mpct_scenario_create changes).
 *   estimator  0: exactly mpct_scenario_create.
 *              MPCT_EST_OUTPUT_BIAS: requires mdband = 1.  desc->plant may differ from desc->model and
 *              nplant > 1 / plant_var ([nplant][my*(nu+nd)], MD columns included) give the plant
 *              draws; simulation s = c*nref + k runs variant k % nplant.  The controller keeps
 *              desc->model and corrects its prediction by the deadbeat output-disturbance observer
 *              (the DMC / IMC bias): b_i(t) = y_i(t) - ym_i(t), ym the model driven from rest by the
 *              applied MVs u(0..t-1) and the measured v(0..t); the QP at step t sees the free
 *              response plus b_i(t) on every row k = 1..N2 of output i, in the tracking term and
 *              the band rows alike.  A stated substitute for the toolbox's default
 *              Kalman estimator, not a restatement of it.  With plant == model b is exactly 0 and
 *              the loop is the nominal one.  dtc and nq > 0 stay rejected.  Closed loop only:
 *              evaluating such a scenario with open_loop = 1 returns MPCT_EINVAL.
 *   any other estimator id, or a non-zero one with mdband = 0: MPCT_EINVAL. */
#define MPCT_EST_OUTPUT_BIAS 1
int32_t mpct_scenario_create_est(const mpct_scenario_desc* desc, int32_t estimator, mpct_scenario** out);
void mpct_scenario_destroy(mpct_scenario* s);

/* Host-table inspection (testing / MATLAB-side debugging; no device needed).
 *   which: 0 = MV step table [my][nu][tlen], 1 = free-response table Phi [my*n2_max][nx],
 *          2 = dims {my, nu, nd, n2_max, nu_max, tlen, nx, nyh, nup, nit, nq},
 *          3 = Phi on the device state basis [y-r, backward differences of y | du history],
 *          4 = the pre-factored prologue rows a device context of this scenario uploads: per
 *              horizon pair (N2 <= n2_max, Nu <= min(N2, nu_max)), in that order, my*min(N2, nu*Nu)
 *              rows of width nu*Nu + nx, row my*k + i = row k of [R_i | T_i] with G_i = Q_i R_i,
 *              T_i = Q_i' Phi_i (table 3's rows).  Empty (0) when the scenario's kernel streams
 *              [G | Phi] instead: not a small plant, more than 16 MiB of rows, or the scenario was
 *              created with the environment variable MPCT_NO_QR_TABLES set to a non-zero number
 *              (the streamed prologue, for comparisons of the two row sources in one process).
 * Copies at most cap doubles into buf; returns the number of doubles the table holds, or <0. */
int64_t mpct_scenario_table(const mpct_scenario* s, int32_t which, double* buf, int64_t cap);

/* Score C candidates x nref references.  Host pointers (MATLAB / ctypes callers).
 *   N2[C], Nu[C]      horizons used by the toolbox: max(N), max(Nu) (closedloop_toolbox.m:38-40)
 *   delta[C*my], lambda[C*nu]   Weights.OV, Weights.MVRate (closedloop_toolbox.m:42-43)
 *   r[nref*my*nit]    reference sets (row signals; VNS passes one unit step per output,
 *                     VNS2.m:148-150; GAM passes Xsp)
 *   v[nref*(nd+nq)*nit] disturbance signals per reference set (NULL when nd + nq == 0)     */
int32_t mpct_eval_batch(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                        const double* delta, const double* lambda, int32_t nref, const double* r,
                        const double* v, const mpct_opts* opts, mpct_result* out);

/* Same, all pointers DEVICE pointers (inputs already resident in HBM; results written to
 * device memory), enqueued on `stream` (a hipStream_t, NULL = default stream) and NOT
 * synchronised — the caller synchronises.  Used by multi-GPU sharding and the benchmark.
 * Batches of 256 or more candidates are dispatched heaviest-first (an a-priori work key and a
 * device radix sort on `stream`, ~20 us; results stay in the caller's order).  The sort buffers
 * belong to the scenario.  Back-to-back calls on one scenario from different streams are safe:
 * each sort waits for the launch that read the previous permutation. */
int32_t mpct_eval_batch_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                               const double* delta, const double* lambda, int32_t nref,
                               const double* r, const double* v, const mpct_opts* opts,
                               mpct_result* out, void* stream);

/* Score C candidates on ndev GPUs of this process at once (host pointers, like mpct_eval_batch).
 * The candidates are independent (VNS2.m:148-169, GAM_fun.m:79-91 score each one in isolation),
 * so they are split into strided shards: slot k scores candidates k, k+ndev, k+2*ndev, ...
 * (mpct_shard_candidates) on devices[k].  Tuning grids are built cell by cell (all lambda draws of
 * one (N2, Nu) pair together), so a contiguous split would hand one slot all the heavy horizons;
 * the strided one gives every slot the same mix.  Each slot gets its own scenario context (a copy
 * of the tables, its own stream and scratch), one host thread per slot gathers its candidates,
 * drives the H2D copies, launch and D2H copies and scatters the results back, and the call returns
 * when every shard is done.  Results land in the caller's order (simulation s = c*nref + k), so a
 * single-threaded MATLAB host drives all GPUs of a node with one call.  A device ordinal may
 * appear more than once (each occurrence gets its own context and stream on that device).
 * ndev = 1 is exactly mpct_eval_batch on devices[0].  opts->device is ignored.  Every ordinal is
 * checked before any work starts.  Errors: the first failing slot's code, its message prefixed
 * with "device <ordinal>: ". */
int32_t mpct_eval_batch_multi(mpct_scenario* s, int32_t ndev, const int32_t* devices, int64_t C,
                              const int32_t* N2, const int32_t* Nu, const double* delta, const double* lambda,
                              int32_t nref, const double* r, const double* v, const mpct_opts* opts,
                              mpct_result* out);

/* The strided shard of C candidates that device slot k of ndev scores (the split of
 * mpct_eval_batch_multi and of the torch.distributed ranks, mpct.dist.shard_indices): candidates
 * k, k+ndev, ... < C.  Writes at most cap indices into idx (idx may be NULL); returns the shard's
 * size ceil((C - k) / ndev), or <0. */
int64_t mpct_shard_candidates(int64_t C, int32_t ndev, int32_t k, int64_t* idx, int64_t cap);

/* The ranking every rank computes after the cost all-gather (Shell3x3.m:161 ranks by
 * the Pareto-weighted cost): perm[0..C) = candidate indices by ascending s_c = sum_j costs[c*k+j] *
 * w[j], ties by candidate index, NaN costs (failed / sentinel candidates) last.  All pointers are
 * DEVICE pointers; enqueued on `stream` (NULL = default), not synchronised.  One key kernel and a
 * device radix sort (stable).  Returns MPCT_OK or <0. */
int32_t mpct_rank_device(const double* costs, int64_t C, int32_t k, const double* w, int32_t* perm, void* stream);

/* Name of the kernel instance mpct_eval_batch(_device) launches for this scenario and options,
 * e.g. "gpc_closed_loop_kernel<16,false,false>" (QP-size class, DTC mode, open-loop/trajectory
 * state).  Copies at most cap-1 characters plus a NUL into buf; returns the name's length, or <0.
 * No device needed (tests pin the instance a benchmark times). */
int32_t mpct_kernel_instance(const mpct_scenario* s, const mpct_opts* opts, char* buf, int32_t cap);

/* Bytes of dynamic LDS one simulation's workgroup uses for this scenario at (N2, Nu) with the
 * open-loop leg / trajectories on (the cost-only instance of a linear scenario needs less); <0 on
 * error.  Lets a host check occupancy before launching. */
int64_t mpct_lds_bytes(const mpct_scenario* s, int32_t N2, int32_t Nu);

/* The same for the instance a call with these options launches (opts NULL = costs only: the
 * GAM_fun.m:81 call, which the tuning-grid benchmark times). */
int64_t mpct_lds_bytes_opts(const mpct_scenario* s, const mpct_opts* opts, int32_t N2, int32_t Nu);

/* ---- Robust scoring over plant draws ----------------------
 * C candidates x D = nref draws, reduced to one record per CANDIDATE on the device.  Simulation
 * (c, k) is candidate c on reference set k and plant variant k % nplant, exactly as in
 * mpct_eval_batch; J(c,k) = sum_i J1_i(c,k) is the draw's total cost.
 *
 * A draw FAILS when its status is non-zero, or J is not finite, or J > j_bound; every other draw
 * SURVIVES.  j_bound = 0 means 1e100; +INFINITY is allowed (then only the status and finiteness
 * decide); a negative or NaN j_bound is MPCT_EINVAL.  A destabilised draw that overflows neither
 * the status nor double precision (a loop at 1e139 keeps status 0) is thus a failed draw of its
 * candidate, never a cost.  A skipped or bad-horizon candidate (MPCT_ST_SKIPPED / _BADHORIZON) has
 * no failed draw: its record carries that status bit, NaN statistics, n_failed = 0, worst_draw = -1.
 *
 * Outputs per candidate; any pointer may be NULL (not all of them):
 *   mean[C*my]     mean over the surviving draws of J1_i; NaN if none survives
 *   worst[C*my]    max over the surviving draws of J1_i; NaN if none survives
 *   n_failed[C]    number of failed draws
 *   worst_draw[C]  the surviving draw with the largest total J, lowest index on ties; -1 if none
 *   status[C]      OR of the draws' status bits (failed draws included)
 *   J1[C*D*my]     optional: the per-simulation costs in mpct_eval_batch's layout, from the same launch
 *
 * Summation order (fixed): per output i one accumulator over the draws k = 0, 1, .., D-1 in that
 * order, divided by the number of survivors; J(c,k) is summed over i = 0, 1, .., my-1.  A repeated
 * call is bitwise identical and a candidate's record does not depend on its place in the batch.
 * With a finite j_bound no statistic can overflow while D * j_bound < 1.8e308 (the default bound:
 * any D), since every surviving term is <= j_bound.  With j_bound = +INFINITY a finite J survives
 * whatever its size and the mean's sum may round to +INFINITY (never NaN: the terms are >= 0).
 *
 * Scenarios the cost-only dtc_small_kernel serves (unconstrained DTC, small plant) with
 * nu * nu_max <= 32 and D <= 128 run the fused dtc_robust_kernel: one workgroup per candidate
 * builds the gain once and walks the draws.  Every other scenario, and D > 128 (the fused kernel's
 * LDS record array), runs its per-simulation instance unchanged and then robust_reduce_kernel; both
 * paths share one reduction, so their records are bitwise equal for equal per-simulation costs. */
typedef struct mpct_robust_result {
  double* mean;
  double* worst;
  int32_t* n_failed;
  int32_t* worst_draw;
  int32_t* status;
  double* J1;
} mpct_robust_result;

/* Host pointers.  Arguments as mpct_eval_batch; the call is cost-only: opts->open_loop or
 * opts->want_traj set is MPCT_EINVAL, as are nref < 1, a bad j_bound and an `out` whose pointers
 * are all NULL.  Without a device: MPCT_EDEVICE with a message, like mpct_eval_batch. */
int32_t mpct_eval_robust(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu, const double* delta,
                         const double* lambda, int32_t nref, const double* r, const double* v, double j_bound,
                         const mpct_opts* opts, mpct_robust_result* out);

/* Same, all pointers DEVICE pointers, enqueued on `stream` (NULL = default stream) and NOT
 * synchronised: the contract of mpct_eval_batch_device, heaviest-first dispatch of batches of 256
 * or more candidates included.  The per-simulation scratch and candidate lists belong to the
 * scenario; a later robust call on another stream waits for the one before it. */
int32_t mpct_eval_robust_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                const double* delta, const double* lambda, int32_t nref, const double* r,
                                const double* v, double j_bound, const mpct_opts* opts, mpct_robust_result* out,
                                void* stream);

/* Name of what a robust call launches for this scenario (at a draw count the fused kernel holds),
 * e.g. "dtc_robust_kernel<16> + dtc_robust_kernel<32>" or "gpc_small_kernel + robust_reduce_kernel".
 * Same buffer contract as mpct_kernel_instance; no device needed. */
int32_t mpct_robust_instance(const mpct_scenario* s, const mpct_opts* opts, char* buf, int32_t cap);

/* ---------------------------------------------------------------------------------------------
 * Tail statistics over the draws: per candidate, empirical quantiles of the total cost J and the mean
 * of the tail above each (CVaR), reduced on the device from the J1 sample of the same launch
 * (robust_tail_kernel, one wave per candidate).  `worst` is the sample maximum (it grows with D and one
 * draw decides it) and `mean` hides the tail; a quantile and its tail mean are what a robust tuner
 * ranks by.
 *
 * For candidate c the draws k = 0 .. D-1 are classified exactly as above: J(k) = sum_i J1_i(k), summed
 * over i = 0 .. my-1 in that order; a draw SURVIVES when its status is 0, J is finite and J <= j_bound
 * (0 means 1e100).  n is the number of survivors; a candidate carrying MPCT_ST_SKIPPED or
 * MPCT_ST_BADHORIZON has n = 0.
 *
 * The survivors are ordered by J ascending and, among equal J, by draw index DESCENDING:
 * J_(1) <= .. <= J_(n).  -0.0 and +0.0 compare equal.  For each level a_j, j = 0 .. nlev-1:
 *   m_j = ceil(a_j * (double)n), evaluated in double arithmetic exactly as written, clamped to [1, n]
 *   quantile[c*nlev+j] = J_(m_j)           the type-1 empirical quantile, no interpolation
 *   q_draw[c*nlev+j]   = the draw index of J_(m_j)
 *   cvar[c*nlev+j]     = (J_(m_j) + J_(m_j+1) + .. + J_(n)) / (n - m_j + 1): one accumulator that starts
 *                        at 0.0 and adds in ascending rank order
 *   n = 0: NaN, NaN, -1.
 *
 * Hence: at level 1.0 quantile = cvar = the largest surviving J and q_draw = worst_draw (the
 * descending tie-break exists for this identity); duplicate levels give identical columns and the
 * levels need not be sorted; a repeated call is bitwise identical and a record does not depend on the
 * candidate's place in the batch.  With a finite bound nothing overflows while D * j_bound < 1.8e308;
 * with j_bound = +INFINITY a tail sum may round to +INFINITY, never NaN.
 *
 * `levels` is a HOST pointer in both entries: a call parameter like j_bound, its values travel to the
 * kernel by value.  `out` may be NULL, or all its pointers NULL, as long as `tail` carries a pointer;
 * the base record written through `out` is bitwise what mpct_eval_robust writes for the same call,
 * and out->J1 is still the optional sample of the same launch (without it the sample lives in the
 * scenario's robust scratch).  The route is mpct_eval_robust's, fused or generic, followed by
 * robust_tail_kernel on the same stream.
 *
 * MPCT_EINVAL, in this order and before any device is touched: nlev < 1 or nlev >
 * MPCT_TAIL_MAX_LEVELS; levels NULL; a level that is NaN, <= 0 or > 1; no result pointer at all in
 * `out` and `tail`; everything mpct_eval_robust rejects.  Then MPCT_ERANGE for nref >
 * MPCT_TAIL_MAX_DRAWS (the kernel stages 12 B of LDS per draw). */
#define MPCT_TAIL_MAX_LEVELS 8
#define MPCT_TAIL_MAX_DRAWS 4096
typedef struct mpct_robust_tail {
  double* quantile; /* [C*nlev] */
  double* cvar;     /* [C*nlev] */
  int32_t* q_draw;  /* [C*nlev]; any of the three may be NULL */
} mpct_robust_tail;

/* Host pointers: mpct_eval_robust plus the tail record. */
int32_t mpct_eval_robust_tail(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu, const double* delta,
                              const double* lambda, int32_t nref, const double* r, const double* v, double j_bound,
                              const mpct_opts* opts, int32_t nlev, const double* levels, mpct_robust_result* out,
                              mpct_robust_tail* tail);

/* Device pointers (levels excepted), enqueued on `stream` and not synchronised: the contract of
 * mpct_eval_robust_device, its stream-ordering rule of the scenario's robust scratch included. */
int32_t mpct_eval_robust_tail_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                     const double* delta, const double* lambda, int32_t nref, const double* r,
                                     const double* v, double j_bound, const mpct_opts* opts, int32_t nlev,
                                     const double* levels, mpct_robust_result* out, mpct_robust_tail* tail,
                                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pareto front, domination counts and non-dominated-sorting layers of a scored grid, on the device
 * (pareto.hip).  mpct_rank_device orders the candidates by one weighted sum, which
 * collapses the objectives and can never return a candidate on a non-convex part of the front; this is
 * its multi-objective counterpart, O(C^2 k) pair tests with exact integer results.
 *
 * costs is [C][k] row-major, the layout mpct_rank_device takes: the J1 per output of mpct_eval_batch, or
 * the mean / worst / quantile / cvar columns of the robust entries.  1 <= k <= MPCT_PARETO_MAX_OBJ,
 * 0 <= C <= MPCT_PARETO_MAX_C.
 *
 * Candidate c is VALID when none of its k costs is NaN.  +-INFINITY are ordinary values (a robust mean
 * may be +INFINITY); -0.0 and +0.0 compare equal.  An invalid candidate dominates nobody and is dominated
 * by nobody: its dom_count and layer are -1 and it is never in front (mpct_rank_device sorts NaN last,
 * RobustResult.scores masks with NaN).
 *
 * a DOMINATES b when both are valid, a_j <= b_j for every j and a_j < b_j for at least one j.  Equal
 * vectors do not dominate each other, so the duplicates of a front point are all on the front.
 *
 *   dom_count[c]   number of valid candidates that dominate c (the Fonseca-Fleming rank; 0 = on the front)
 *   front[0 .. n_front)  the valid candidates with dom_count 0, in ascending candidate index;
 *                  front[n_front .. C) = -1, so the caller's buffer of C entries is fully defined
 *   n_front[0]     the size of the front
 *   layer[c]       the non-dominated-sorting layer: 0 on the front, else 1 + the largest layer among c's
 *                  dominators (peeling the front off repeatedly), computed for max_layers = L layers,
 *                  1 <= L <= MPCT_PARETO_MAX_LAYERS: a valid candidate deeper than layer L - 1 gets exactly L
 *                  ("beyond")
 * Any of the four pointers may be NULL, not all of them; n_front alone is fine.  A repeated call is bitwise
 * identical; permuting the candidates permutes dom_count and layer and maps the front's set of indices.
 *
 * Argument errors, in this order and before any device is touched:
 *   MPCT_EINVAL  k < 1 or k > MPCT_PARETO_MAX_OBJ
 *   MPCT_EINVAL  C < 0
 *   MPCT_ERANGE  C > MPCT_PARETO_MAX_C
 *   MPCT_EINVAL  costs NULL (with C > 0)
 *   MPCT_EINVAL  out NULL, or all four of its pointers NULL
 *   MPCT_EINVAL  front without n_front
 *   MPCT_EINVAL  max_layers < 0 or > MPCT_PARETO_MAX_LAYERS, or layer non-NULL with max_layers = 0
 * C = 0 writes n_front[0] = 0 and returns MPCT_OK. */
#define MPCT_PARETO_MAX_OBJ 16
#define MPCT_PARETO_MAX_C 1048576
#define MPCT_PARETO_MAX_LAYERS 64
typedef struct mpct_pareto_result {
  int32_t* dom_count; /* [C] */
  int32_t* layer;     /* [C] */
  int32_t* front;     /* [C] */
  int32_t* n_front;   /* [1] */
} mpct_pareto_result;

/* All pointers DEVICE pointers, n_front included; enqueued on `stream` (NULL = default stream) and NOT
 * synchronised.  Scratch comes from hipMallocAsync / hipFreeAsync on that stream, as in mpct_rank_device,
 * so calls on different streams are independent.  The work is bounded by C, k and max_layers alone:
 * exactly max_layers counting passes are enqueued with no host synchronisation; a pass with no
 * candidate left leaves at once. */
int32_t mpct_pareto_device(const double* costs, int64_t C, int32_t k, int32_t max_layers,
                           const mpct_pareto_result* out, void* stream);

/* Host pointers (MATLAB and C callers); needs no scenario.  device: HIP ordinal, -1 = the current device
 * (an ordinal out of range is MPCT_EINVAL).  Stages on a stream of its own and waits for that stream only;
 * the calling thread's current device is unchanged on return.  Without a device: MPCT_EDEVICE with a message. */
int32_t mpct_pareto(const double* costs, int64_t C, int32_t k, int32_t max_layers, int32_t device,
                    const mpct_pareto_result* out);

/* ---------------------------------------------------------------------------------------------
 * Hypervolume of a set of cost vectors inside a box, and every member's exclusive contribution, on the
 * device (hypervolume.hip).  mpct_pareto ends in a front that is too large to read; this
 * says how good a front is (the volume of the box it dominates: compare two fronts in one box) and which
 * of its members matter (the volume a member alone dominates: 0 = redundant, the largest = the knees).
 * Exact hypervolume is exponential in k, so this is a Monte-Carlo estimate over a counter-based sample
 * set: N points x M members x k column tests, and every result an integer count.
 *
 * costs is [C][k] row-major, mpct_pareto's table: 1 <= k <= MPCT_PARETO_MAX_OBJ, 0 <= C <= MPCT_PARETO_MAX_C.
 * members[M] are int32 indices into costs, 0 <= M <= MPCT_PARETO_MAX_C.  members NULL means candidates
 * 0 .. C-1, and then M must equal C.  An entry -1 is SKIPPED, so the -1-padded front of mpct_pareto may
 * be passed as it is with M = C.  Any other entry outside [0, C) is MPCT_EINVAL for mpct_hypervolume,
 * which reads the entries on the host; mpct_hypervolume_device cannot see them before it enqueues and
 * treats such an entry as skipped.  A duplicated index counts twice.
 *
 * lo[k], ref[k] are the box: every value finite and lo[j] < ref[j].  n_samples = N, 1 <= N <=
 * MPCT_HV_MAX_SAMPLES; seed is any uint64.
 *
 * A member row with a NaN among its k costs covers nothing (mpct_pareto's validity rule); +-INFINITY are
 * ordinary values; -0.0 equals +0.0.
 *
 * SAMPLE POINTS, part of the contract, in uint64 arithmetic that wraps.  Point i in [0, N), column j in [0, k):
 *     x = seed + 0x9E3779B97F4A7C15 * (16*i + j + 1)
 *     x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9
 *     x ^= x >> 27;  x *= 0x94D049BB133111EB
 *     x ^= x >> 31
 *     u   = (double)(x >> 11) * 2^-53
 *     p_j = lo_j + u * (ref_j - lo_j)
 * with the difference and the product each rounded to double before the sum (no fused multiply-add).
 *
 * Member a COVERS point p when a_j <= p_j for every j < k.  depth(p) is the number of entries of members,
 * neither skipped nor NaN, that cover p.
 *
 *   n_covered[0]    number of points with depth >= 1
 *   excl[m]         number of points with depth exactly 1 whose one covering entry is members[m]; 0 for a
 *                   skipped or NaN entry; equal vectors cover the same points, so each of them gets 0
 *   depth_hist[b]   number of points with depth 0, 1, .., 6 and (b = 7) >= 7: how much the members overlap
 *   hv[0]           ((double)n_covered / (double)N) * vol, vol the product over ascending j of (ref_j - lo_j)
 *                   starting from 1.0, every factor and product rounded
 * Any of the four pointers may be NULL, not all of them.  A repeated call is bitwise identical; a
 * permutation of members permutes excl and changes nothing else; no result depends on the launch geometry.
 *
 * Argument errors, in this order and before any device is touched:
 *   MPCT_EINVAL  k < 1 or k > MPCT_PARETO_MAX_OBJ
 *   MPCT_EINVAL  C < 0 or M < 0
 *   MPCT_ERANGE  C or M > MPCT_PARETO_MAX_C
 *   MPCT_ERANGE  n_samples > MPCT_HV_MAX_SAMPLES
 *   MPCT_EINVAL  n_samples < 1
 *   MPCT_EINVAL  costs NULL (with M > 0)
 *   MPCT_EINVAL  members NULL with M != C
 *   MPCT_EINVAL  lo or ref NULL
 *   MPCT_EINVAL  out NULL, or all four of its pointers NULL
 *   MPCT_EINVAL  (mpct_hypervolume only) a value of lo or ref not finite, or lo[j] >= ref[j]
 *   MPCT_EINVAL  (mpct_hypervolume only) an entry of members below -1 or >= C
 * The last two read the caller's arrays, which only the host entry can do: mpct_hypervolume_device writes
 * hv[0] = NaN for such a box (the counts are then whatever the comparisons give) and skips such an entry.
 * M = 0 is legal: every count is 0, depth_hist[0] = N and hv[0] follows from n_covered = 0. */
#define MPCT_HV_MAX_SAMPLES 1073741824
#define MPCT_HV_BINS 8
typedef struct mpct_hv_result {
  int64_t* n_covered;  /* [1] */
  int64_t* excl;       /* [M] */
  int64_t* depth_hist; /* [MPCT_HV_BINS] */
  double* hv;          /* [1] */
} mpct_hv_result;

/* All pointers DEVICE pointers, lo, ref and the outputs included; enqueued on `stream` (NULL = default
 * stream) and NOT synchronised.  Scratch comes from hipMallocAsync / hipFreeAsync on that stream, as in
 * mpct_pareto_device, so calls on different streams are independent.  The work is bounded by N, M and k alone. */
int32_t mpct_hypervolume_device(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M,
                                const double* lo, const double* ref, int64_t n_samples, uint64_t seed,
                                const mpct_hv_result* out, void* stream);

/* Host pointers (MATLAB and C callers); needs no scenario.  device: HIP ordinal, -1 = the current device
 * (an ordinal out of range is MPCT_EINVAL).  Stages on a stream of its own and waits for that stream only;
 * the calling thread's current device is unchanged on return.  M = 0 needs no device.  Without a device:
 * MPCT_EDEVICE with a message. */
int32_t mpct_hypervolume(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M,
                         const double* lo, const double* ref, int64_t n_samples, uint64_t seed, int32_t device,
                         const mpct_hv_result* out);

/* ---------------------------------------------------------------------------------------------
 * Hypervolume subset selection: the n members that carry a front, by greedy forward selection on the
 * coverage count, on the device (hv_select.hip).  excl of mpct_hypervolume says what a member
 * alone dominates with every other member present, so two near-duplicate knees hide each other and a short
 * list of the largest excl can miss whole regions of the trade-off.  This call picks, round by round, the
 * member that covers the most sample points no earlier pick covers.  The count is monotone and submodular,
 * so the first n picks cover at least 1 - (1 - 1/n)^n of what the best n-subset covers of the same sample
 * set, and the gains order the members so that the list may be cut anywhere.
 *
 * costs, C, k, members, M, lo, ref, n_samples and seed are mpct_hypervolume's, with its sample points, its
 * coverage rule, NaN rows and -1 entries that cover nothing, +-INFINITY as ordinary values, -0.0 equal to
 * +0.0 and a duplicated index as a separate entry.  n_pick = K is the number of rounds, 1 <= K <=
 * MPCT_HVSEL_MAX_PICKS; K may exceed M.
 *
 * U_0 is all N points.  Round r = 0 .. K-1: gain_r(m) = #{i in U_r : members[m] covers p_i}.  If the largest
 * gain is 0 the selection ENDS: n_picked = r, and the slots r .. K-1 hold the fill stated below.  Otherwise
 * m_r is the smallest m with the largest gain, and U_(r+1) = U_r minus the points m_r covers.
 *
 *   n_picked[0]       rounds that picked a member
 *   pos[r]            m_r, the position in members of round r's pick; -1 after the end
 *   index[r]          members[m_r] (m_r when members is NULL); -1 after the end
 *   gain[r]           points newly covered by round r's pick; 0 after the end
 *   covered[r]        gain[0] + .. + gain[r]; stays at its last value after the end (0 when nothing was picked)
 *   hv[r]             ((double)covered[r] / (double)N) * vol, vol as in mpct_hypervolume
 *   ties[r]           entries of members that held round r's largest gain (1: the pick was forced); 0 after the end
 *   n_covered_all[0]  points covered by any entry: mpct_hypervolume's n_covered
 * Any of the eight pointers may be NULL, not all of them.  A repeated call is bitwise identical; no result
 * depends on the launch geometry; gain is non-increasing; if the selection ends before K,
 * covered[n_picked - 1] == n_covered_all; where every ties[r] == 1, a permutation of members leaves index,
 * gain, covered and hv unchanged and permutes pos.
 *
 * Argument errors, in this order and before any device is touched:
 *   MPCT_EINVAL  k < 1 or k > MPCT_PARETO_MAX_OBJ
 *   MPCT_EINVAL  C < 0 or M < 0
 *   MPCT_ERANGE  C or M > MPCT_PARETO_MAX_C
 *   MPCT_ERANGE  n_samples > MPCT_HV_MAX_SAMPLES
 *   MPCT_EINVAL  n_samples < 1
 *   MPCT_EINVAL  n_pick < 1
 *   MPCT_ERANGE  n_pick > MPCT_HVSEL_MAX_PICKS
 *   MPCT_EINVAL  costs NULL (with M > 0)
 *   MPCT_EINVAL  members NULL with M != C
 *   MPCT_EINVAL  lo or ref NULL
 *   MPCT_EINVAL  out NULL, or all eight of its pointers NULL
 *   MPCT_EINVAL  (mpct_hv_select only) a value of lo or ref not finite, or lo[j] >= ref[j]
 *   MPCT_EINVAL  (mpct_hv_select only) an entry of members below -1 or >= C
 * As for mpct_hypervolume, only the host entry can read the caller's arrays: mpct_hv_select_device writes
 * hv[r] = NaN for such a box and skips such an entry.  M = 0 is legal: n_picked = 0 and every slot holds
 * the fill. */
#define MPCT_HVSEL_MAX_PICKS 1024
typedef struct mpct_hv_select_result {
  int64_t* n_picked;      /* [1]  rounds that picked a member                                   */
  int32_t* pos;           /* [K]  position m_r in members of round r's pick; -1 after the end   */
  int32_t* index;         /* [K]  members[m_r] (m_r when members is NULL); -1 after the end     */
  int64_t* gain;          /* [K]  points newly covered by round r's pick; 0 after the end       */
  int64_t* covered;       /* [K]  gain[0] + .. + gain[r]; stays at its last value after the end */
  double*  hv;            /* [K]  ((double)covered[r] / (double)N) * vol, vol as in mpct_hypervolume */
  int32_t* ties;          /* [K]  entries of members that held round r's maximal gain (1 = the pick was forced); 0 after the end */
  int64_t* n_covered_all; /* [1]  points covered by any entry: mpct_hypervolume's n_covered     */
} mpct_hv_select_result;

/* All pointers DEVICE pointers, lo, ref and the outputs included; enqueued on `stream` (NULL = default
 * stream) and NOT synchronised: a fixed sequence of launches that depends on n_pick, n_samples and M only.
 * Scratch (the per-member gains and one "still uncovered" bit per point, 128 MiB at N = 2^30) comes from
 * hipMallocAsync / hipFreeAsync on that stream, so calls on different streams are independent. */
int32_t mpct_hv_select_device(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M,
                              const double* lo, const double* ref, int64_t n_samples, uint64_t seed, int32_t n_pick,
                              const mpct_hv_select_result* out, void* stream);

/* Host pointers (MATLAB and C callers); needs no scenario.  device: HIP ordinal, -1 = the current device
 * (an ordinal out of range is MPCT_EINVAL).  Stages on a stream of its own and waits for that stream only;
 * the calling thread's current device is unchanged on return.  M = 0 needs no device.  Without a device:
 * MPCT_EDEVICE with a message. */
int32_t mpct_hv_select(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M,
                       const double* lo, const double* ref, int64_t n_samples, uint64_t seed, int32_t n_pick,
                       int32_t device, const mpct_hv_select_result* out);

/* ---------------------------------------------------------------------------------------------
 * Exact hypervolume and exclusive contributions for at most three objectives, on the device
 * (hypervolume_exact.hip).  mpct_hypervolume's estimate has a standard error of about 1e-3 of
 * the box at 2^20 points and reads every contribution below 1/N of the box as 0.  For k <= 3 a sweep gives
 * the volume and every contribution with rounding error only, in O(M^2) work and with no sample count.
 *
 * costs, C, members, M, lo and ref are mpct_hypervolume's: costs is [C][k] row-major, members NULL means
 * candidates 0 .. C-1 with M = C, an entry -1 is SKIPPED (the -1-padded front of mpct_pareto goes in as it
 * is with M = C), a duplicated index is a separate entry, and an entry outside [0, C) is MPCT_EINVAL for
 * mpct_hypervolume_exact and skipped by mpct_hypervolume_exact_device.  1 <= k <= MPCT_HVX_MAX_OBJ,
 * 0 <= C <= MPCT_PARETO_MAX_C, 0 <= M <= MPCT_HVX_MAX_M.
 *
 * An entry whose row holds a NaN is INACTIVE.  Every other entry a is clipped to the box, b_j = max(a_j, lo_j)
 * (-INFINITY clips to lo_j; -0.0 equals +0.0), and is inactive when b_j >= ref_j for some j (+INFINITY, or a
 * member on or past a reference face).  Every other entry is ACTIVE and owns the box [b, ref).
 *
 *   hv[0]        the Lebesgue measure of the union of the active boxes: what mpct_hypervolume estimates
 *   excl[m]      the measure of the part of entry m's box that lies in no other active entry's box; +0.0 for
 *                an inactive entry and for each of two entries with equal clipped vectors
 *   n_active[0]  the number of active entries
 * Any of the three pointers may be NULL, not all of them.  M = 0, or no active entry: hv = +0.0, n_active = 0.
 *
 * ARITHMETIC, part of the contract.  IEEE doubles, every operation rounded (no fused multiply-add).  Every term
 * that enters a sum is a product of non-negative differences of clipped coordinates; no volume is obtained by
 * subtraction.  With T = M*M + 8, vol the box volume of mpct_hypervolume and HV, EXCL_m the values in exact
 * arithmetic on the doubles given:  |hv - HV| <= T * 2^-53 * vol  and  |excl[m] - EXCL_m| <= T * 2^-53 * vol.
 * excl[m] is exactly +0.0 where EXCL_m is 0.  Where every difference, product and partial sum is representable
 * (small integer coordinates, scaled by a power of two or not) every result is exact.  A repeated call is bitwise
 * identical; no result depends on C, on where the rows sit in costs, or on the launch geometry; a permutation
 * of members permutes excl bitwise and leaves hv and n_active bitwise unchanged (the order of every sum is a
 * function of the sorted clipped values alone).
 *
 * Argument errors, in this order and before any device is touched:
 *   MPCT_EINVAL  k < 1
 *   MPCT_ERANGE  k > MPCT_HVX_MAX_OBJ
 *   MPCT_EINVAL  C < 0 or M < 0
 *   MPCT_ERANGE  C > MPCT_PARETO_MAX_C
 *   MPCT_ERANGE  M > MPCT_HVX_MAX_M
 *   MPCT_EINVAL  costs NULL (with M > 0)
 *   MPCT_EINVAL  members NULL with M != C
 *   MPCT_EINVAL  lo or ref NULL
 *   MPCT_EINVAL  out NULL, or all three of its pointers NULL
 *   MPCT_EINVAL  (mpct_hypervolume_exact only) a value of lo or ref not finite, or lo[j] >= ref[j]
 *   MPCT_EINVAL  (mpct_hypervolume_exact only) an entry of members below -1 or >= C
 * The last two read the caller's arrays, which only the host entry can do: mpct_hypervolume_exact_device
 * writes hv = NaN and excl = NaN for such a box (n_active = 0) and skips such an entry. */
#define MPCT_HVX_MAX_OBJ 3
#define MPCT_HVX_MAX_M   65536
typedef struct mpct_hvx_result {
  double*  hv;        /* [1] volume of the box dominated by any member            */
  double*  excl;      /* [M] volume dominated by members[m] and by no other entry */
  int64_t* n_active;  /* [1] entries whose clipped box has positive volume        */
} mpct_hvx_result;

/* All pointers DEVICE pointers, lo, ref and the outputs included; enqueued on `stream` (NULL = default
 * stream) and NOT synchronised: a fixed sequence of launches that depends on M and k only.  Scratch (at most
 * 256 * M * 8 bytes, 128 MiB at M = MPCT_HVX_MAX_M) comes from hipMallocAsync / hipFreeAsync on that stream,
 * so calls on different streams are independent. */
int32_t mpct_hypervolume_exact_device(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M,
                                      const double* lo, const double* ref, const mpct_hvx_result* out, void* stream);

/* Host pointers (MATLAB and C callers); needs no scenario.  device: HIP ordinal, -1 = the current device
 * (an ordinal out of range is MPCT_EINVAL).  Stages on a stream of its own and waits for that stream only;
 * the calling thread's current device is unchanged on return.  M = 0 needs no device.  Without a device:
 * MPCT_EDEVICE with a message. */
int32_t mpct_hypervolume_exact(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M,
                               const double* lo, const double* ref, int32_t device, const mpct_hvx_result* out);

/* ---------------------------------------------------------------------------------------------
 * Closed-loop performance indices per simulation, reduced on the device from the trajectories
 * (traj_indices.hip): what a control engineer reads off the plots of the reference's drivers
 * -- integrated errors, overshoot, settling time, valve travel, peak move -- as columns for mpct_pareto or
 * mpct_rank_device, without the trajectories leaving the device.
 *
 * Trajectories in mpct_result's layout: y[S][my][nit], u[S][nu][nit], r[nref][my][nit]; simulation s reads
 * reference set s % nref (S is a multiple of nref).  The indices cover the samples t = t0 .. nit-1.
 *
 * Output row (s, i), with e(t) = y(t) - r(t), r_f = r(nit-1), d = r_f - y(t0), sigma = sign(d) (0 for d = 0):
 *   iae      sum_t |e(t)|
 *   ise      sum_t e(t)*e(t)
 *   itae     sum_t (double)(t - t0) * |e(t)|
 *   emax     max_t |e(t)|;  t_emax  the first t that attains it
 *   over     sigma != 0: the excursion past the reference in the step's direction, max_t sigma*e(t) where that
 *            is > 0, else +0.0.  sigma = 0 (a regulated or interaction channel): emax
 *   e_final  e(nit-1), signed
 *   settle   the smallest T in [t0, nit] with |y(t) - r_f| <= band for every t >= T, where
 *            band = band_rel*|d| + band_abs: the last violating sample + 1, t0 when there is none, and
 *            nit = "not settled at the last sample"
 * Input row (s, n), with du(t) = u(t) - u(t-1) for t = t0+1 .. nit-1:
 *   tv       sum |du|         du2    sum du*du        dumax  max |du|; the three are 0.0 over an empty range
 *   u_lo, u_hi  min and max of u(t), t >= t0; a zero extreme is +0.0 whatever the signs of the row's zeros
 *
 * Row validity.  A row is VALID when every sample it reads in [t0, nit) is finite: y and r for an output
 * row, u for an input row.  An invalid row gives NaN in every double field and -1 in every integer field;
 * other rows are not affected.  This covers the NaN trajectories of MPCT_ST_SKIPPED, MPCT_ST_BADHORIZON and
 * MPCT_ST_NOT_RUN slots; samples before t0 are never read.
 *
 * No contraction.  Every product above is rounded to double before it is added (e*e, (t-t0)*|e|, du*du and
 * band_rel*|d|): no fused multiply-add anywhere, so a host restatement in plain IEEE double arithmetic gives
 * the same bits -- one fused operation in `band` could move `settle` by a sample.
 *
 * Summation order (fixed).  Lane l = (t - t0) mod 64 accumulates its samples in ascending t, starting from
 * 0.0; a lane without a sample keeps 0.0.  The 64 partials p0 .. p63 are then combined as a pairwise tree in
 * lane order: (p0 + p1), (p2 + p3), ..; then ((p0 + p1) + (p2 + p3)), ..; up to (p0..p31) + (p32..p63).
 * A repeated call is bitwise identical and a record does not depend on the simulation's place in the
 * batch.  Maxima, minima, t_emax and settle are exact whatever the order.
 *
 * Any result pointer may be NULL, but not all of them.  y and r may be NULL when no output-row field is
 * requested, u when no input-row field is.  Only the requested arrays are written, and only their S rows.
 *
 * Argument errors, in this order and before any device is touched:
 *   MPCT_EINVAL  params NULL; S < 0, my < 0, nu < 0 or nit < 1
 *   MPCT_EINVAL  nref < 1
 *   MPCT_EINVAL  S not a multiple of nref
 *   MPCT_EINVAL  t0 < 0 or t0 >= nit
 *   MPCT_EINVAL  band_rel or band_abs negative, infinite or NaN
 *   MPCT_EINVAL  out NULL, or all thirteen of its pointers NULL
 *   MPCT_EINVAL  an output-row field with my < 1, or (S > 0) with y or r NULL; an input-row field with
 *                nu < 1, or (S > 0) with u NULL
 *   MPCT_ERANGE  S*my or S*nu > MPCT_INDEX_MAX_ROWS (one wave per row, four rows per workgroup)
 * S = 0 is MPCT_OK and writes nothing. */
#define MPCT_INDEX_MAX_ROWS 2147483647
typedef struct mpct_index_params {
  int32_t t0;      /* first sample of the indices, 0 <= t0 < nit */
  double band_rel; /* settling band relative to the step size |d| (0.02 = the 2 % band) */
  double band_abs; /* plus an absolute band; both finite and >= 0 */
} mpct_index_params;

typedef struct mpct_index_result {
  double* iae;      /* [S*my] */
  double* ise;      /* [S*my] */
  double* itae;     /* [S*my] */
  double* emax;     /* [S*my] */
  int32_t* t_emax;  /* [S*my] */
  double* over;     /* [S*my] */
  double* e_final;  /* [S*my] */
  int32_t* settle;  /* [S*my] */
  double* tv;       /* [S*nu] */
  double* du2;      /* [S*nu] */
  double* dumax;    /* [S*nu] */
  double* u_lo;     /* [S*nu] */
  double* u_hi;     /* [S*nu] */
} mpct_index_result;

/* All pointers DEVICE pointers; enqueued on `stream` (NULL = default stream) and NOT synchronised.  Needs no
 * scenario and no scratch: one kernel launch. */
int32_t mpct_indices_device(const double* y, const double* u, const double* r, int64_t S, int32_t nref, int32_t my,
                            int32_t nu, int32_t nit, const mpct_index_params* params, const mpct_index_result* out,
                            void* stream);

/* Host pointers (MATLAB and C callers), for trajectories from any source, MATLAB's own sim included.
 * device: HIP ordinal, -1 = the current device (an ordinal out of range is MPCT_EINVAL).  Stages on a stream
 * of its own and waits for that stream only; the calling thread's current device is unchanged on return.
 * Without a device: MPCT_EDEVICE with a message. */
int32_t mpct_indices(const double* y, const double* u, const double* r, int64_t S, int32_t nref, int32_t my, int32_t nu,
                     int32_t nit, const mpct_index_params* params, int32_t device, const mpct_index_result* out);

/* Score a batch and return only the index records (host pointers; arguments as mpct_eval_batch).  The
 * closed loops run with their trajectories written to device scratch that belongs to the scenario's context,
 * traj_indices_kernel reduces them there on the same stream, and only the records travel back: S = C*nref
 * simulations, output rows [S*my], input rows [S*nu]; the reference sets of the indices are the call's r.
 *   res   optional: J1, j21, j22, Jnu, status and qp_iters of the same launch (j21 and Jnu come back NaN: the
 *         call is closed-loop only).  Its trajectory pointers y, u, ys, uopt must be NULL.
 *   opts  open_loop = 1 is MPCT_EINVAL; want_traj is ignored (the call sets it).
 * Chunking.  The trajectory scratch is bounded by MPCT_INDEX_SCRATCH_BYTES (or one candidate's trajectories,
 * nref*(my+nu)*nit*8 bytes, where that is more): the batch is walked in chunks of whole candidates, each
 * chunk's launch followed by the index kernel on the same stream.  Every record is bitwise independent of
 * the chunk size.
 * MPCT_EINVAL, in this order and before any device is touched: s NULL; params NULL; open_loop set; a
 * trajectory pointer in res; then everything mpct_eval_batch rejects; then the checks of mpct_indices_device
 * from t0 on.  C = 0 is MPCT_OK and writes nothing.  Without a device: MPCT_EDEVICE with a message. */
#define MPCT_INDEX_SCRATCH_BYTES 268435456 /* 256 MiB */
int32_t mpct_eval_indices(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu, const double* delta,
                          const double* lambda, int32_t nref, const double* r, const double* v, const mpct_opts* opts,
                          const mpct_index_params* params, mpct_result* res, const mpct_index_result* out);

/* Same, all pointers DEVICE pointers (res's and out's included), enqueued on `stream` (NULL = default
 * stream) and NOT synchronised: the contract of mpct_eval_batch_device.  The trajectory scratch belongs to
 * the scenario; a later call on another stream waits for the one before it, and a regrow waits for the work
 * on the old buffer before freeing it. */
int32_t mpct_eval_indices_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu, const double* delta,
                                 const double* lambda, int32_t nref, const double* r, const double* v,
                                 const mpct_opts* opts, const mpct_index_params* params, mpct_result* res,
                                 const mpct_index_result* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Robust index statistics: per-candidate statistics of any per-simulation table over its draws, on the
 * device (draw_stats.hip).  mpct_eval_robust reduces the C x D simulations of a plant-mismatch
 * Monte-Carlo for the tracking cost only and the index entries give one record per simulation; these give
 * what a robust tuner ranks by -- the worst overshoot over the draws, a quantile of the settling time, the
 * CVaR of the valve travel -- one number per candidate and channel, as columns for mpct_pareto.
 *
 * The primitive.  x is [C][D][m] row-major, the layout of every per-simulation array of this library
 * (simulation s = c*D + k: J1[s*my+i], iae[s*my+i], tv[s*nu+n]); x_type is MPCT_STAT_F64 (double) or
 * MPCT_STAT_I32 (int32, converted to double exactly; a negative value is "no value", the -1 of an invalid
 * index row).  alive is [C][D] or NULL (every draw alive).  Draw k SURVIVES in column (c, i) when alive is
 * NULL or alive[c*D+k] != 0, and the value is finite (F64) or >= 0 (I32).  The columns are independent;
 * n is the column's number of survivors.
 *
 * Per column, element c*m + i of each array:
 *   n         the survivor count
 *   mean      one accumulator from 0.0 over the surviving draws in ascending k, divided by (double)n
 *   lo, lo_draw   the smallest surviving value and the lowest draw index that holds it
 *   hi, hi_draw   the largest surviving value and the lowest draw index that holds it
 *             lo and hi carry the bits of the value at lo_draw / hi_draw; -0.0 and +0.0 compare equal
 * Per column and level j, element (c*m + i)*nlev + j: quantile, cvar, q_draw, defined as in
 * mpct_eval_robust_tail on the column's survivors: ordered by value ascending and, among equal values, by
 * draw index DESCENDING; m_j = ceil(a_j * (double)n) clamped to [1, n]; quantile the value of rank m_j
 * (type 1, no interpolation), q_draw its draw, cvar = (sum of ranks m_j .. n) / (n - m_j + 1) with one
 * accumulator from 0.0 in ascending rank order.
 * n = 0: NaN in the doubles, -1 in the draws.  At level 1.0 quantile = cvar = hi and q_draw = hi_draw;
 * duplicate levels give equal columns and the levels need not be sorted.  A repeated call is bitwise
 * identical and a column's record depends neither on C nor on its place in the table.
 * Any pointer of mpct_draw_stats_result may be NULL, not all of them.  levels is a HOST pointer in both entries;
 * nlev may be 0.
 *
 * Argument errors, in this order and before any device is touched:
 *   MPCT_EINVAL  C < 0, D < 1 or m < 1
 *   MPCT_EINVAL  x_type neither MPCT_STAT_F64 nor MPCT_STAT_I32
 *   MPCT_EINVAL  nlev < 0 or nlev > MPCT_TAIL_MAX_LEVELS
 *   MPCT_EINVAL  nlev > 0 with levels NULL
 *   MPCT_EINVAL  a level that is NaN, <= 0 or > 1
 *   MPCT_EINVAL  out NULL, or all nine of its pointers NULL
 *   MPCT_EINVAL  a quantile, cvar or q_draw pointer with nlev = 0
 *   MPCT_EINVAL  x NULL with C > 0
 *   MPCT_ERANGE  D > MPCT_TAIL_MAX_DRAWS (12 B of LDS per draw)
 *   MPCT_ERANGE  C*m > MPCT_INDEX_MAX_ROWS
 * C = 0 is MPCT_OK and writes nothing. */
#define MPCT_STAT_F64 0
#define MPCT_STAT_I32 1
typedef struct mpct_draw_stats_result {
  int32_t* n;        /* [C*m] */
  double* mean;      /* [C*m] */
  double* lo;        /* [C*m] */
  int32_t* lo_draw;  /* [C*m] */
  double* hi;        /* [C*m] */
  int32_t* hi_draw;  /* [C*m] */
  double* quantile;  /* [C*m*nlev] */
  double* cvar;      /* [C*m*nlev] */
  int32_t* q_draw;   /* [C*m*nlev] */
} mpct_draw_stats_result;

/* All pointers DEVICE pointers (levels excepted); enqueued on `stream` (NULL = default stream) and NOT
 * synchronised.  Needs no scenario and no scratch: one kernel launch. */
int32_t mpct_draw_stats_device(const void* x, int32_t x_type, const int32_t* alive, int64_t C, int32_t D, int32_t m,
                               int32_t nlev, const double* levels, const mpct_draw_stats_result* out, void* stream);

/* Host pointers (MATLAB and C callers).  device: HIP ordinal, -1 = the current device (an ordinal out of range
 * is MPCT_EINVAL).  Stages on a stream of its own and waits for that stream only; the calling thread's current
 * device is unchanged on return.  Without a device: MPCT_EDEVICE with a message. */
int32_t mpct_draw_stats(const void* x, int32_t x_type, const int32_t* alive, int64_t C, int32_t D, int32_t m,
                        int32_t nlev, const double* levels, int32_t device, const mpct_draw_stats_result* out);

/* Score C candidates x D = nref draws and return, per candidate, the statistics over the draws of the
 * selected performance indices (host pointers; arguments as mpct_eval_indices and mpct_eval_robust).
 *   fields   HOST pointer to nsel distinct field ids, MPCT_IX_IAE .. MPCT_IX_U_HI in the member order of
 *            mpct_index_result.  The selected fields lie side by side in selection order: W = sum of their
 *            widths (my for an output-row field, nu for an input-row field), and every array of `out` is
 *            [C][W] or [C][W][nlev] -- out->hi is directly a cost table for mpct_pareto_device.  t_emax and
 *            settle enter as MPCT_STAT_I32, the others as MPCT_STAT_F64.
 *   levels   HOST pointer, nlev may be 0 (then out's quantile, cvar and q_draw must be NULL).
 *   base     optional: mean and worst of J1, n_failed, worst_draw and status exactly as mpct_eval_robust
 *            defines them, from the same launch.  base->J1 must be NULL: the sample lives per chunk.
 * Per chunk of whole candidates (the chunking of mpct_eval_indices, MPCT_INDEX_SCRATCH_BYTES of trajectory
 * scratch) the closed loops run with their trajectories, J1 and status written to scratch of the scenario's
 * context; traj_indices_kernel reduces the selected fields to per-simulation records there; a classify kernel
 * writes alive[c][k] by the rule of mpct_eval_robust (status 0, J = sum_i J1_i finite, summed over
 * i = 0 .. my-1 in that order, J <= j_bound with 0 = 1e100; a candidate carrying MPCT_ST_SKIPPED or
 * MPCT_ST_BADHORIZON on any draw has no live draw); and the primitive above runs once per selected field.
 * A draw also drops out of a column whose record is invalid (NaN / -1).  Every record is bitwise independent
 * of the chunk size.
 * Errors, in this order and before any device is touched.  MPCT_EINVAL: s NULL; params NULL; open_loop
 * set; nsel < 1 or > 13, fields NULL, an id out of range or repeated; nref < 1; a negative or NaN j_bound;
 * nlev < 0 or > MPCT_TAIL_MAX_LEVELS, nlev > 0 with levels NULL, a level that is NaN, <= 0 or > 1; no result
 * pointer at all in `base` and `out`, base->J1 set, or a quantile / cvar / q_draw pointer with nlev = 0; then
 * everything mpct_eval_batch rejects; then t0 or the bands as in mpct_indices_device.  Then MPCT_ERANGE for
 * nref > MPCT_TAIL_MAX_DRAWS, and for C*nref*my or C*nref*nu > MPCT_INDEX_MAX_ROWS.
 * C = 0 is MPCT_OK and writes nothing.  Without a device: MPCT_EDEVICE with a message. */
#define MPCT_IX_IAE 0
#define MPCT_IX_ISE 1
#define MPCT_IX_ITAE 2
#define MPCT_IX_EMAX 3
#define MPCT_IX_T_EMAX 4
#define MPCT_IX_OVER 5
#define MPCT_IX_E_FINAL 6
#define MPCT_IX_SETTLE 7
#define MPCT_IX_TV 8
#define MPCT_IX_DU2 9
#define MPCT_IX_DUMAX 10
#define MPCT_IX_U_LO 11
#define MPCT_IX_U_HI 12
int32_t mpct_eval_robust_indices(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu, const double* delta,
                                 const double* lambda, int32_t nref, const double* r, const double* v, double j_bound,
                                 const mpct_opts* opts, const mpct_index_params* params, int32_t nsel,
                                 const int32_t* fields, int32_t nlev, const double* levels, mpct_robust_result* base,
                                 const mpct_draw_stats_result* out);

/* Same, all pointers DEVICE pointers except fields and levels, enqueued on `stream` (NULL = default stream)
 * and NOT synchronised: the contract of mpct_eval_indices_device, whose scratch and stream-ordering rule it
 * shares (grow-only; a regrow waits for the work on the old buffer; a call on another stream waits for an
 * event recorded after the previous call's last kernel). */
int32_t mpct_eval_robust_indices_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                        const double* delta, const double* lambda, int32_t nref, const double* r,
                                        const double* v, double j_bound, const mpct_opts* opts,
                                        const mpct_index_params* params, int32_t nsel, const int32_t* fields,
                                        int32_t nlev, const double* levels, mpct_robust_result* base,
                                        const mpct_draw_stats_result* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Limit indices per simulation, reduced on the device from the trajectories (limit_indices.hip; DESIGN.md
 * §20): the counterpart of the performance indices for bounds instead of a reference -- how far, how long and
 * how late an output was outside its band [y_lo, y_hi] (zone control), and how much of a run the inputs spent
 * at their amplitude bounds [u_lo, u_hi] or at their rate bounds [du_lo, du_hi] -- as columns for mpct_pareto
 * or mpct_rank_device, without the trajectories leaving the device.
 *
 * Trajectories in mpct_result's layout: y[S][my][nit], u[S][nu][nit].  The indices cover the samples
 * t = t0 .. nit-1.  Bounds are per channel: y_lo, y_hi [my]; u_lo, u_hi, du_lo, du_hi [nu]; a lower bound may be
 * -inf and an upper bound +inf (no bound on that side).  Every subtraction below is rounded once.
 *
 * Output row (s, i), with m(t) = max(y_lo - y(t), y(t) - y_hi) and ex(t) = m(t) where m(t) > 0, else +0.0
 * (that is fmax(fmax(y_lo - y, y - y_hi), 0.0) with a zero that is always +0.0):
 *   viol      sum_t ex(t)
 *   viol2     sum_t ex(t)*ex(t)
 *   vmax      max_t ex(t);  t_vmax  the first t that attains it (t0 when ex is 0 throughout)
 *   n_out     the number of samples with ex(t) > out_tol
 *   t_in      the last sample with ex(t) > out_tol, plus one; t0 when there is none; nit = "still outside at
 *             the last sample"
 *   y_margin  min_t min(y(t) - y_lo, y_hi - y(t)): negative once the band is violated, +inf without a bound; a
 *             zero margin is +0.0
 * Input row (s, n), with du(t) = u(t) - u(t-1) for t = t0+1 .. nit-1; sample t is AT-LO when
 * u(t) - u_lo <= sat_tol and AT-HI when u_hi - u(t) <= sat_tol:
 *   n_lo, n_hi  the number of at-lo and of at-hi samples, t >= t0
 *   n_rate      the number of samples t >= t0+1 with du(t) - du_lo <= sat_tol or du_hi - du(t) <= sat_tol
 *   sat_run     the longest run of consecutive samples that are at-lo or at-hi (0 when there is none)
 *   u_margin    min_t min(u(t) - u_lo, u_hi - u(t)), t >= t0; +inf without a bound; a zero margin is +0.0
 *   du_margin   min_t min(du(t) - du_lo, du_hi - du(t)), t >= t0+1; +inf without a bound or over an empty range
 *
 * Row validity.  As for the performance indices: a row is VALID when every sample it reads in [t0, nit) is
 * finite.  An invalid row gives NaN in every double field and -1 in every integer field; other rows are not
 * affected; samples before t0 are never read.
 *
 * No contraction.  ex*ex is rounded to double before it is added: no fused multiply-add anywhere.
 *
 * Summation order (fixed), that of the performance indices.  Lane l = (t - t0) mod 64 accumulates its samples
 * in ascending t, starting from 0.0; the 64 partials are combined as a pairwise tree in lane order, up to
 * (p0..p31) + (p32..p63).  Counts, maxima, minima, t_vmax, t_in and sat_run are exact whatever the order, and
 * sat_run is exact across the 64-sample blocks.  A repeated call is bitwise identical and a record does not
 * depend on the simulation's place in the batch.
 *
 * The parameter struct and the six arrays it points to are HOST memory in every entry, the _device ones
 * included, and are read before the call returns (they travel by value in the kernel argument).  In the two
 * scenario-free entries a NULL array means no bound (-inf / +inf).
 *
 * Any result pointer may be NULL, but not all of them.  y may be NULL when no output-row field is requested,
 * u when no input-row field is.  Only the requested arrays are written, and only their S rows.
 *
 * Argument errors, in this order and before any device is touched:
 *   MPCT_EINVAL  params NULL; S < 0, my < 0, nu < 0 or nit < 1
 *   MPCT_EINVAL  t0 < 0 or t0 >= nit
 *   MPCT_ERANGE  my or nu > MPCT_LIMIT_MAX_CH (the bounds travel in the kernel argument)
 *   MPCT_EINVAL  out_tol or sat_tol negative, infinite or NaN
 *   MPCT_EINVAL  a bound that is NaN; a lower bound above its upper bound; a lower bound of +inf or an upper
 *                bound of -inf
 *   MPCT_EINVAL  out NULL, or all thirteen of its pointers NULL
 *   MPCT_EINVAL  an output-row field with my < 1, or (S > 0) with y NULL; an input-row field with nu < 1, or
 *                (S > 0) with u NULL
 *   MPCT_ERANGE  S*my or S*nu > MPCT_INDEX_MAX_ROWS (one wave per row, four rows per workgroup)
 * S = 0 is MPCT_OK and writes nothing. */
#define MPCT_LIMIT_MAX_CH 32
typedef struct mpct_limit_params {
  int32_t t0;          /* first sample of the indices, 0 <= t0 < nit */
  double out_tol;      /* an output sample counts as outside when ex > out_tol; finite and >= 0 */
  double sat_tol;      /* an input sample counts as at a bound within sat_tol of it; finite and >= 0 */
  const double* y_lo;  /* [my] HOST, or NULL */
  const double* y_hi;  /* [my] */
  const double* u_lo;  /* [nu] */
  const double* u_hi;  /* [nu] */
  const double* du_lo; /* [nu] */
  const double* du_hi; /* [nu] */
} mpct_limit_params;

typedef struct mpct_limit_result {
  double* viol;       /* [S*my] */
  double* viol2;      /* [S*my] */
  double* vmax;       /* [S*my] */
  int32_t* t_vmax;    /* [S*my] */
  int32_t* n_out;     /* [S*my] */
  int32_t* t_in;      /* [S*my] */
  double* y_margin;   /* [S*my] */
  int32_t* n_lo;      /* [S*nu] */
  int32_t* n_hi;      /* [S*nu] */
  int32_t* n_rate;    /* [S*nu] */
  int32_t* sat_run;   /* [S*nu] */
  double* u_margin;   /* [S*nu] */
  double* du_margin;  /* [S*nu] */
} mpct_limit_result;

/* the field ids of mpct_eval_robust_limit_indices, in the member order of mpct_limit_result */
#define MPCT_LX_VIOL 0
#define MPCT_LX_VIOL2 1
#define MPCT_LX_VMAX 2
#define MPCT_LX_T_VMAX 3
#define MPCT_LX_N_OUT 4
#define MPCT_LX_T_IN 5
#define MPCT_LX_Y_MARGIN 6
#define MPCT_LX_N_LO 7
#define MPCT_LX_N_HI 8
#define MPCT_LX_N_RATE 9
#define MPCT_LX_SAT_RUN 10
#define MPCT_LX_U_MARGIN 11
#define MPCT_LX_DU_MARGIN 12

/* y, u and the pointers of `out` DEVICE pointers (params and its arrays HOST); enqueued on `stream` (NULL =
 * default stream) and NOT synchronised.  Needs no scenario and no scratch: one kernel launch. */
int32_t mpct_limit_indices_device(const double* y, const double* u, int64_t S, int32_t my, int32_t nu, int32_t nit,
                                  const mpct_limit_params* params, const mpct_limit_result* out, void* stream);

/* Host pointers (MATLAB and C callers), for trajectories from any source.  device: HIP ordinal, -1 = the
 * current device (an ordinal out of range is MPCT_EINVAL).  Stages on a stream of its own and waits for that
 * stream only; y travels only behind an output-row field and u only behind an input-row field; the calling
 * thread's current device is unchanged on return.  Without a device: MPCT_EDEVICE with a message. */
int32_t mpct_limit_indices(const double* y, const double* u, int64_t S, int32_t my, int32_t nu, int32_t nit,
                           const mpct_limit_params* params, int32_t device, const mpct_limit_result* out);

/* Score a batch and return only the limit records (host pointers; arguments as mpct_eval_indices, whose
 * chunking, scratch, `res` and `opts` rules hold unchanged): S = C*nref simulations, output rows [S*my], input
 * rows [S*nu].  A NULL array of params takes the scenario's own bound: du_min, du_max, u_min and u_max of its
 * descriptor (an NMPC scenario has u_min and u_max only), y_min and y_max of an mdband scenario; whatever the
 * scenario does not hold is -inf / +inf.  Every record is bitwise independent of the chunk size.
 * MPCT_EINVAL, in this order and before any device is touched: s NULL; params NULL; open_loop set; a
 * trajectory pointer in res; then everything mpct_eval_batch rejects; then the checks of
 * mpct_limit_indices_device from t0 on, the bounds as resolved.  C = 0 is MPCT_OK and writes nothing.  Without
 * a device: MPCT_EDEVICE with a message. */
int32_t mpct_eval_limit_indices(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu, const double* delta,
                                const double* lambda, int32_t nref, const double* r, const double* v,
                                const mpct_opts* opts, const mpct_limit_params* params, mpct_result* res,
                                const mpct_limit_result* out);

/* Same, all pointers DEVICE pointers (res's and out's included; params and its arrays HOST), enqueued on
 * `stream` (NULL = default stream) and NOT synchronised: the contract of mpct_eval_indices_device, whose
 * scratch and stream-ordering rule it shares. */
int32_t mpct_eval_limit_indices_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                       const double* delta, const double* lambda, int32_t nref, const double* r,
                                       const double* v, const mpct_opts* opts, const mpct_limit_params* params,
                                       mpct_result* res, const mpct_limit_result* out, void* stream);

/* Score C candidates x D = nref draws and return, per candidate, the statistics over the draws of the
 * selected limit indices: the arguments and semantics of mpct_eval_robust_indices with mpct_limit_params in
 * place of mpct_index_params (a NULL array: the scenario's own bound, as in mpct_eval_limit_indices) and
 * `fields` drawn from MPCT_LX_VIOL .. MPCT_LX_DU_MARGIN.  The int32 fields enter the statistics as
 * MPCT_STAT_I32, the others as MPCT_STAT_F64; an infinite margin (no bound) is a draw without a value, by the
 * statistics' own rule.  Per chunk: the closed loops with trajectories, limit_indices_kernel for the selected
 * fields only, the classify kernel, the statistics per field and the base record.
 * Errors, in this order and before any device is touched: those of mpct_eval_robust_indices up to and
 * including everything mpct_eval_batch rejects; then t0, the channel cap (MPCT_ERANGE), the tolerances and the
 * resolved bounds as in mpct_limit_indices_device; then MPCT_ERANGE for nref > MPCT_TAIL_MAX_DRAWS, and for
 * C*nref*my or C*nref*nu > MPCT_INDEX_MAX_ROWS.  C = 0 is MPCT_OK and writes nothing. */
int32_t mpct_eval_robust_limit_indices(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                       const double* delta, const double* lambda, int32_t nref, const double* r,
                                       const double* v, double j_bound, const mpct_opts* opts,
                                       const mpct_limit_params* params, int32_t nsel, const int32_t* fields,
                                       int32_t nlev, const double* levels, mpct_robust_result* base,
                                       const mpct_draw_stats_result* out);

/* Same, all pointers DEVICE pointers except params with its arrays, fields and levels; enqueued on `stream`
 * and NOT synchronised: the contract of mpct_eval_robust_indices_device. */
int32_t mpct_eval_robust_limit_indices_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                              const double* delta, const double* lambda, int32_t nref,
                                              const double* r, const double* v, double j_bound,
                                              const mpct_opts* opts, const mpct_limit_params* params, int32_t nsel,
                                              const int32_t* fields, int32_t nlev, const double* levels,
                                              mpct_robust_result* base, const mpct_draw_stats_result* out,
                                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * Step-response indices per setpoint segment, reduced on the device from the trajectories
 * (segment_indices.hip).  The performance indices above measure overshoot and settling time
 * against ONE step per run, r_f = r(nit-1) and d = r_f - y(t0); a scenario whose reference changes several
 * times (Shell 3x3: samples 9, 79, 199, 399, and back to 0) has d = 0 there.  These entries cut the run into
 * segments at the setpoint changes and give one record per (row, segment): the indices above per segment,
 * plus the rise time and the undershoot of an inverse response.
 *
 * Segments.  nseg in [1, MPCT_SEG_MAX]; tseg[nseg+1] is a HOST pointer to strictly ascending int32 with
 * 0 <= tseg[0] and tseg[nseg] <= nit.  Segment g covers the samples a <= t < b with a = tseg[g], b = tseg[g+1].
 * One boundary list serves every row and every reference set; the boundaries travel to the kernel by value in
 * its argument.  Nothing before tseg[0] or from tseg[nseg] on is ever read.
 *
 * Trajectories in mpct_result's layout: y[S][my][nit], u[S][nu][nit], r[nref][my][nit]; simulation s reads
 * reference set s % nref (S is a multiple of nref).
 *
 * Output row (s, i), segment g, with e(t) = y(t) - r(t) and r_g = r(b-1).  The base level c: in segment 0
 * c = y(a), whatever `base`; in a later segment c = y(a) with base = 0 (the rule of the performance indices)
 * and c = r(a-1), the level the reference left, with base = 1.  d = r_g - c, sigma = sign(d) (0 for d = 0),
 * p(t) = sigma*(y(t) - c):
 *   iae      sum_t |e(t)|
 *   ise      sum_t e(t)*e(t)
 *   itae     sum_t (double)(t - a) * |e(t)|
 *   emax     max_t |e(t)|;  t_emax  the first t that attains it (an absolute sample)
 *   over     sigma != 0: max_t sigma*e(t) where that is > 0, else +0.0.  sigma = 0: emax
 *   under    the excursion on the wrong side of the base level (inverse response).  sigma != 0: max_t -p(t)
 *            where that is > 0, else +0.0.  sigma = 0: +0.0
 *   e_final  e(b-1), signed
 *   settle   the smallest T in [a, b] with |y(t) - r_g| <= band_rel*|d| + band_abs for every t in [T, b): the
 *            last violating sample + 1, a when there is none; b = "not settled inside the segment"
 *   rise     t_hi - t_lo, where t_lo / t_hi are the first t in [a, b) with p(t) >= rise_lo*|d| /
 *            p(t) >= rise_hi*|d|; b - a when sigma != 0 and t_hi does not exist; -1 when sigma = 0
 * Input row (s, n), segment g, with du(t) = u(t) - u(t-1) for t in [max(a, tseg[0]+1), b): the move across a
 * boundary belongs to the segment it starts, so over real numbers the segments' tv add up to the whole run's:
 *   tv       sum |du|         du2    sum du*du        dumax  max |du|; the three are 0.0 over an empty range
 *   u_lo, u_hi  min and max of u(t) over [a, b); a zero extreme is +0.0
 *
 * Layout.  Element (row*nseg + g) of each array: output fields [S][my][nseg], input fields [S][nu][nseg].
 *
 * Validity.  The unit is one (row, segment).  It is INVALID when any sample it reads is non-finite: y and r in
 * [a, b), and r(a-1) where base = 1 uses it (g >= 1), for an output unit; u in [a, b), and u(a-1) for g >= 1,
 * for an input unit.  An invalid unit gives NaN in its doubles and -1 in its integers; no other unit is
 * affected, the other segments of the same row included.
 *
 * No contraction; fixed order.  Every product above is rounded to double before it is added (e*e,
 * (t-a)*|e|, du*du, band_rel*|d|, rise_lo*|d|, rise_hi*|d|): no fused multiply-add anywhere.  Lane
 * l = (t - a) mod 64 accumulates its samples in ascending t, starting from 0.0; the 64 partials are combined
 * as the pairwise tree in lane order of the performance indices.  Extremes, t_emax, settle and rise are
 * exact.  A repeated call is bitwise identical and a record does not depend on the simulation's place in the
 * batch.
 *
 * Consequence.  With nseg = 1, base = 0 and tseg = {t0, nit}, every field shared with mpct_index_result (all
 * but under and rise) equals that of mpct_indices_device with the same t0, band_rel and band_abs bit for bit.
 *
 * Any result pointer may be NULL, but not all of them.  y and r may be NULL when no output-row field is
 * requested, u when no input-row field is.  Only the requested arrays are written.
 *
 * Argument errors, in this order and before any device is touched:
 *   MPCT_EINVAL  params NULL; S < 0, my < 0, nu < 0 or nit < 1
 *   MPCT_EINVAL  nref < 1
 *   MPCT_EINVAL  S not a multiple of nref
 *   MPCT_EINVAL  nseg < 1 or tseg NULL
 *   MPCT_ERANGE  nseg > MPCT_SEG_MAX (the boundaries travel in the kernel argument)
 *   MPCT_EINVAL  tseg[0] < 0, tseg[nseg] > nit, or tseg not strictly ascending
 *   MPCT_EINVAL  base neither 0 nor 1
 *   MPCT_EINVAL  band_rel or band_abs negative, infinite or NaN
 *   MPCT_EINVAL  rise_lo or rise_hi NaN, or not 0 <= rise_lo <= rise_hi <= 1
 *   MPCT_EINVAL  out NULL, or all fifteen of its pointers NULL
 *   MPCT_EINVAL  an output-row field with my < 1, or (S > 0) with y or r NULL; an input-row field with
 *                nu < 1, or (S > 0) with u NULL
 *   MPCT_ERANGE  S*my*nseg or S*nu*nseg > MPCT_INDEX_MAX_ROWS (one wave per row and segment)
 * S = 0 is MPCT_OK and writes nothing. */
#define MPCT_SEG_MAX 16
typedef struct mpct_segment_params {
  int32_t nseg;        /* 1 .. MPCT_SEG_MAX */
  const int32_t* tseg; /* [nseg+1] HOST, strictly ascending, 0 <= tseg[0], tseg[nseg] <= nit */
  int32_t base;        /* base level of segments g >= 1: 0 = y(a), 1 = r(a-1) */
  double band_rel;     /* settling band relative to the step size |d| */
  double band_abs;     /* plus an absolute band; both finite and >= 0 */
  double rise_lo;      /* rise levels as fractions of |d| (0.1 and 0.9: the 10-90 % rise time); */
  double rise_hi;      /* 0 <= rise_lo <= rise_hi <= 1 */
} mpct_segment_params;

typedef struct mpct_segment_result {
  double* iae;      /* [S*my*nseg] */
  double* ise;      /* [S*my*nseg] */
  double* itae;     /* [S*my*nseg] */
  double* emax;     /* [S*my*nseg] */
  int32_t* t_emax;  /* [S*my*nseg] */
  double* over;     /* [S*my*nseg] */
  double* under;    /* [S*my*nseg] */
  double* e_final;  /* [S*my*nseg] */
  int32_t* settle;  /* [S*my*nseg] */
  int32_t* rise;    /* [S*my*nseg] */
  double* tv;       /* [S*nu*nseg] */
  double* du2;      /* [S*nu*nseg] */
  double* dumax;    /* [S*nu*nseg] */
  double* u_lo;     /* [S*nu*nseg] */
  double* u_hi;     /* [S*nu*nseg] */
} mpct_segment_result;

/* the field ids of mpct_eval_robust_segment_indices, in the member order of mpct_segment_result */
#define MPCT_SX_IAE 0
#define MPCT_SX_ISE 1
#define MPCT_SX_ITAE 2
#define MPCT_SX_EMAX 3
#define MPCT_SX_T_EMAX 4
#define MPCT_SX_OVER 5
#define MPCT_SX_UNDER 6
#define MPCT_SX_E_FINAL 7
#define MPCT_SX_SETTLE 8
#define MPCT_SX_RISE 9
#define MPCT_SX_TV 10
#define MPCT_SX_DU2 11
#define MPCT_SX_DUMAX 12
#define MPCT_SX_U_LO 13
#define MPCT_SX_U_HI 14

/* The segment boundaries of a reference, on the host (no device): {0} u {t >= 1 where any row of any
 * reference set has r(t) != r(t-1)} u the caller's `extra` event samples u {nit}, sorted and deduplicated,
 * into tseg_out[0 .. *nseg].  r is [nref][my][nit]; `extra` (nextra values, or NULL with nextra = 0) carries
 * instants the reference does not show, such as the sample of a measured disturbance; tseg_out holds
 * max_seg + 1 values.  MPCT_EINVAL, in this order: r, tseg_out or nseg NULL; nref < 1, my < 1 or nit < 1;
 * max_seg < 1; nextra < 0, or nextra > 0 with extra NULL; an extra sample outside [0, nit]; a non-finite r.
 * More than max_seg segments: MPCT_ERANGE (nothing is written). */
int32_t mpct_reference_segments(const double* r, int32_t nref, int32_t my, int32_t nit, const int32_t* extra,
                                int32_t nextra, int32_t max_seg, int32_t* tseg_out, int32_t* nseg);

/* y, u, r and the pointers of `out` DEVICE pointers (params and its tseg HOST, read before the call returns);
 * enqueued on `stream` (NULL = default stream) and NOT synchronised.  Needs no scenario and no scratch: one
 * kernel launch. */
int32_t mpct_segment_indices_device(const double* y, const double* u, const double* r, int64_t S, int32_t nref,
                                    int32_t my, int32_t nu, int32_t nit, const mpct_segment_params* params,
                                    const mpct_segment_result* out, void* stream);

/* Host pointers (MATLAB and C callers), for trajectories from any source.  device: HIP ordinal, -1 = the
 * current device (an ordinal out of range is MPCT_EINVAL).  Stages on a stream of its own and waits for that
 * stream only; y and r travel only behind an output-row field and u only behind an input-row field; the
 * calling thread's current device is unchanged on return.  Without a device: MPCT_EDEVICE with a message. */
int32_t mpct_segment_indices(const double* y, const double* u, const double* r, int64_t S, int32_t nref, int32_t my,
                             int32_t nu, int32_t nit, const mpct_segment_params* params, int32_t device,
                             const mpct_segment_result* out);

/* Score a batch and return only the segment records (host pointers; arguments as mpct_eval_indices, whose
 * chunking, scratch, `res` and `opts` rules hold unchanged): S = C*nref simulations, output fields
 * [S*my*nseg], input fields [S*nu*nseg]; the reference sets of the indices are the call's r.  Every record is
 * bitwise independent of the chunk size.
 * MPCT_EINVAL, in this order and before any device is touched: s NULL; params NULL; open_loop set; a
 * trajectory pointer in res; then everything mpct_eval_batch rejects; then the checks of
 * mpct_segment_indices_device from nseg on, nit the scenario's.  C = 0 is MPCT_OK and writes nothing.  Without a
 * device: MPCT_EDEVICE with a message. */
int32_t mpct_eval_segment_indices(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                  const double* delta, const double* lambda, int32_t nref, const double* r,
                                  const double* v, const mpct_opts* opts, const mpct_segment_params* params,
                                  mpct_result* res, const mpct_segment_result* out);

/* Same, all pointers DEVICE pointers (res's and out's included; params and its tseg HOST), enqueued on
 * `stream` (NULL = default stream) and NOT synchronised: the contract of mpct_eval_indices_device, whose
 * scratch and stream-ordering rule it shares. */
int32_t mpct_eval_segment_indices_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                         const double* delta, const double* lambda, int32_t nref, const double* r,
                                         const double* v, const mpct_opts* opts, const mpct_segment_params* params,
                                         mpct_result* res, const mpct_segment_result* out, void* stream);

/* Score C candidates x D = nref draws and return, per candidate, the statistics over the draws of the
 * selected segment indices: the arguments and semantics of mpct_eval_robust_indices with mpct_segment_params
 * in place of mpct_index_params and `fields` drawn from MPCT_SX_IAE .. MPCT_SX_U_HI (1 <= nsel <= 15).  A
 * selected output-row field contributes my*nseg columns (channel i, segment g at i*nseg + g), an input-row
 * field nu*nseg: the tables of `out` are [C][W] and [C][W][nlev] with W the sum over the selection.  t_emax,
 * settle and rise enter the statistics as MPCT_STAT_I32, so a rise of -1 (sigma = 0) is a draw without a
 * value; the others as MPCT_STAT_F64.  `base` is the robust J1 record of the same launch.
 * Errors, in this order and before any device is touched: those of mpct_eval_robust_indices up to and
 * including everything mpct_eval_batch rejects; then the checks of mpct_segment_indices_device from nseg up
 * to rise_hi; then MPCT_ERANGE for nref > MPCT_TAIL_MAX_DRAWS, and for C*nref*my*nseg or C*nref*nu*nseg >
 * MPCT_INDEX_MAX_ROWS.  C = 0 is MPCT_OK and writes nothing. */
int32_t mpct_eval_robust_segment_indices(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                         const double* delta, const double* lambda, int32_t nref, const double* r,
                                         const double* v, double j_bound, const mpct_opts* opts,
                                         const mpct_segment_params* params, int32_t nsel, const int32_t* fields,
                                         int32_t nlev, const double* levels, mpct_robust_result* base,
                                         const mpct_draw_stats_result* out);

/* Same, all pointers DEVICE pointers except params with its tseg, fields and levels; enqueued on `stream`
 * and NOT synchronised: the contract of mpct_eval_robust_indices_device. */
int32_t mpct_eval_robust_segment_indices_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                                const double* delta, const double* lambda, int32_t nref,
                                                const double* r, const double* v, double j_bound,
                                                const mpct_opts* opts, const mpct_segment_params* params,
                                                int32_t nsel, const int32_t* fields, int32_t nlev,
                                                const double* levels, mpct_robust_result* base,
                                                const mpct_draw_stats_result* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Oscillation indices per setpoint segment, reduced on the device from the trajectories
 * (osc_indices.hip).  The segment indices above say how far, how long and how late a closed
 * loop misses its target; none of them says whether it RINGS.  One clean overshoot that dies and a lightly
 * damped loop that crosses its setpoint six times can share `over`, `settle` and much of `iae`.  These entries
 * count the band crossings of each output in each segment, give the decay ratio and the period of its first two
 * peaks on one side and the peak of its last lobe, and count the direction reversals of each input (the valve
 * wear figure beside tv).
 *
 * Segments.  Exactly those of mpct_segment_params: nseg in [1, MPCT_SEG_MAX]; tseg[nseg+1] is a HOST pointer to
 * strictly ascending int32 with 0 <= tseg[0] and tseg[nseg] <= nit.  Segment g covers the samples a <= t < b
 * with a = tseg[g], b = tseg[g+1].  mpct_reference_segments gives the boundaries of a reference; they travel to
 * the kernel by value in its argument.  Nothing before tseg[0] or from tseg[nseg] on is ever read.
 *
 * Trajectories in mpct_result's layout: y[S][my][nit], u[S][nu][nit], r[nref][my][nit]; simulation s reads
 * reference set s % nref (S is a multiple of nref).
 *
 * Output row (s, i), segment g.  r_g = r(b-1), the base level c (segment 0: y(a); later: y(a) with base = 0,
 * r(a-1) with base = 1), d = r_g - c and sigma = sign(d) exactly as in the segment indices.  x(t) = y(t) - r_g
 * is measured against the segment's final level, not against r(t).  h = band_rel*|d| + band_abs, the product
 * rounded before the sum.  The STATE of a sample is +1 if x(t) > h, -1 if x(t) < -h, else INSIDE (|x| == h is
 * inside).  Walk the OUTSIDE samples in ascending t:
 *   - a CROSSING is an outside sample whose state differs from that of the previous outside sample, however
 *     many inside samples lie between them; the first outside sample is no crossing;
 *   - LOBE k (k = 0, 1, ..) is the set of outside samples after the k-th crossing and before the (k+1)-th (lobe
 *     0: before the first), A_k the largest |x| in lobe k, T_k the first t that attains A_k.
 * k0 = 1 when sigma != 0 (lobe 0 is then the approach to the new level), k0 = 0 otherwise (a disturbance or a
 * hold: lobe 0 is the first excursion).
 *   ncross   the number of crossings
 *   decay    A_{k0+2} / A_{k0}, one IEEE division, when ncross >= k0 + 2; else +0.0 (no second peak on the same
 *            side left the band)
 *   period   T_{k0+2} - T_{k0} when ncross >= k0 + 2; else -1
 *   a_last   A_ncross, the peak of the last lobe, when ncross >= k0; else +0.0; +0.0 as well when no sample
 *            is outside (an empty lobe has no peak).  A loop whose a_last is near A_{k0} oscillates undamped;
 *            above it, it grows
 * Input row (s, n), segment g, with the moves du(t) = u(t) - u(t-1) for t in [max(a, tseg[0]+1), b), the range
 * of the segment indices (the move across a boundary belongs to the segment it starts).  The state of a move
 * is +1 if du > rev_tol, -1 if du < -rev_tol, else inside:
 *   nmove    the number of outside moves
 *   nrev     the number of crossings among the outside moves, as above: the direction reversals
 *   t_rev    the sample t of the last reversing move; -1 when nrev = 0
 *
 * Layout.  Element (row*nseg + g) of each array: output fields [S][my][nseg], input fields [S][nu][nseg].
 *
 * Validity.  The unit is one (row, segment).  It is INVALID when any sample it reads is non-finite.  An output
 * unit reads y in [a, b), r(b-1), and r(a-1) where base = 1 uses it (g >= 1); no other sample of r: x does
 * not involve r(t).  An input unit reads u in [a, b), and u(a-1) for g >= 1.  An invalid unit gives NaN in its
 * doubles and -1 in its integers; no other unit is affected, the other segments of the same row included.
 *
 * Exact; no contraction.  Every field is an exact integer or a bit-exact double: the doubles are maxima of |x|
 * and one division; there is no sum, so no summation order.  band_rel*|d| is rounded to double before band_abs
 * is added: no fused multiply-add.  -0.0 counts as +0.0 in every comparison (rev_tol = 0: a move of +-0.0 is
 * inside).  A repeated call is bitwise identical and a record does not depend on the simulation's place in the
 * batch.
 *
 * Any result pointer may be NULL, but not all of them.  y and r may be NULL when no output-row field is
 * requested, u when no input-row field is.  Only the requested arrays are written.
 *
 * Argument errors, in this order and before any device is touched:
 *   MPCT_EINVAL  params NULL; S < 0, my < 0, nu < 0 or nit < 1
 *   MPCT_EINVAL  nref < 1
 *   MPCT_EINVAL  S not a multiple of nref
 *   MPCT_EINVAL  nseg < 1 or tseg NULL
 *   MPCT_ERANGE  nseg > MPCT_SEG_MAX (the boundaries travel in the kernel argument)
 *   MPCT_EINVAL  tseg[0] < 0, tseg[nseg] > nit, or tseg not strictly ascending
 *   MPCT_EINVAL  base neither 0 nor 1
 *   MPCT_EINVAL  band_rel or band_abs negative, infinite or NaN
 *   MPCT_EINVAL  rev_tol negative, infinite or NaN
 *   MPCT_EINVAL  out NULL, or all seven of its pointers NULL
 *   MPCT_EINVAL  an output-row field with my < 1, or (S > 0) with y or r NULL; an input-row field with
 *                nu < 1, or (S > 0) with u NULL
 *   MPCT_ERANGE  S*my*nseg or S*nu*nseg > MPCT_INDEX_MAX_ROWS (one wave per row and segment)
 * S = 0 is MPCT_OK and writes nothing. */
typedef struct mpct_osc_params {
  int32_t nseg;        /* 1 .. MPCT_SEG_MAX */
  const int32_t* tseg; /* [nseg+1] HOST, strictly ascending, 0 <= tseg[0], tseg[nseg] <= nit */
  int32_t base;        /* base level of segments g >= 1: 0 = y(a), 1 = r(a-1) */
  double band_rel;     /* band around r_g relative to the step size |d| */
  double band_abs;     /* plus an absolute band; both finite and >= 0 */
  double rev_tol;      /* dead zone of a move: |du| <= rev_tol is no move; finite and >= 0 */
} mpct_osc_params;

typedef struct mpct_osc_result {
  int32_t* ncross;  /* [S*my*nseg] */
  double* decay;    /* [S*my*nseg] */
  int32_t* period;  /* [S*my*nseg] */
  double* a_last;   /* [S*my*nseg] */
  int32_t* nmove;   /* [S*nu*nseg] */
  int32_t* nrev;    /* [S*nu*nseg] */
  int32_t* t_rev;   /* [S*nu*nseg] */
} mpct_osc_result;

/* the field ids of mpct_eval_robust_osc_indices, in the member order of mpct_osc_result */
#define MPCT_OX_NCROSS 0
#define MPCT_OX_DECAY 1
#define MPCT_OX_PERIOD 2
#define MPCT_OX_A_LAST 3
#define MPCT_OX_NMOVE 4
#define MPCT_OX_NREV 5
#define MPCT_OX_T_REV 6

/* y, u, r and the pointers of `out` DEVICE pointers (params and its tseg HOST, read before the call returns);
 * enqueued on `stream` (NULL = default stream) and NOT synchronised.  Needs no scenario and no scratch: one
 * kernel launch. */
int32_t mpct_osc_indices_device(const double* y, const double* u, const double* r, int64_t S, int32_t nref,
                                int32_t my, int32_t nu, int32_t nit, const mpct_osc_params* params,
                                const mpct_osc_result* out, void* stream);

/* Host pointers (MATLAB and C callers), for trajectories from any source: the staging, device and stream
 * rules of mpct_segment_indices.  Without a device: MPCT_EDEVICE with a message. */
int32_t mpct_osc_indices(const double* y, const double* u, const double* r, int64_t S, int32_t nref, int32_t my,
                         int32_t nu, int32_t nit, const mpct_osc_params* params, int32_t device,
                         const mpct_osc_result* out);

/* Score a batch and return only the oscillation records (host pointers; arguments as
 * mpct_eval_segment_indices, whose chunking, scratch, `res` and `opts` rules hold unchanged): S = C*nref
 * simulations, output fields [S*my*nseg], input fields [S*nu*nseg]; the reference sets of the indices are the
 * call's r.  Every record is bitwise independent of the chunk size.
 * MPCT_EINVAL, in this order and before any device is touched: s NULL; params NULL; open_loop set; a
 * trajectory pointer in res; then everything mpct_eval_batch rejects; then the checks of
 * mpct_osc_indices_device from nseg on, nit the scenario's.  C = 0 is MPCT_OK and writes nothing.  Without a
 * device: MPCT_EDEVICE with a message. */
int32_t mpct_eval_osc_indices(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu, const double* delta,
                              const double* lambda, int32_t nref, const double* r, const double* v,
                              const mpct_opts* opts, const mpct_osc_params* params, mpct_result* res,
                              const mpct_osc_result* out);

/* Same, all pointers DEVICE pointers (res's and out's included; params and its tseg HOST), enqueued on
 * `stream` (NULL = default stream) and NOT synchronised: the contract of mpct_eval_segment_indices_device. */
int32_t mpct_eval_osc_indices_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                     const double* delta, const double* lambda, int32_t nref, const double* r,
                                     const double* v, const mpct_opts* opts, const mpct_osc_params* params,
                                     mpct_result* res, const mpct_osc_result* out, void* stream);

/* Score C candidates x D = nref draws and return, per candidate, the statistics over the draws of the
 * selected oscillation indices: the arguments and semantics of mpct_eval_robust_segment_indices with
 * mpct_osc_params in place of mpct_segment_params and `fields` drawn from MPCT_OX_NCROSS .. MPCT_OX_T_REV
 * (1 <= nsel <= 7).  A selected output-row field contributes my*nseg columns (channel i, segment g at
 * i*nseg + g), an input-row field nu*nseg.  ncross, period, nmove, nrev and t_rev enter the statistics as
 * MPCT_STAT_I32, so a period or a t_rev of -1 is a draw without a value; decay and a_last as MPCT_STAT_F64.
 * The worst decay and the upper quantiles of ncross over the draws stand beside the worst overshoot.
 * Errors, in this order and before any device is touched: those of mpct_eval_robust_indices up to and
 * including everything mpct_eval_batch rejects; then the checks of mpct_osc_indices_device from nseg up to
 * rev_tol; then MPCT_ERANGE for nref > MPCT_TAIL_MAX_DRAWS, and for C*nref*my*nseg or C*nref*nu*nseg >
 * MPCT_INDEX_MAX_ROWS.  C = 0 is MPCT_OK and writes nothing. */
int32_t mpct_eval_robust_osc_indices(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                     const double* delta, const double* lambda, int32_t nref, const double* r,
                                     const double* v, double j_bound, const mpct_opts* opts,
                                     const mpct_osc_params* params, int32_t nsel, const int32_t* fields,
                                     int32_t nlev, const double* levels, mpct_robust_result* base,
                                     const mpct_draw_stats_result* out);

/* Same, all pointers DEVICE pointers except params with its tseg, fields and levels; enqueued on `stream`
 * and NOT synchronised: the contract of mpct_eval_robust_indices_device. */
int32_t mpct_eval_robust_osc_indices_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                            const double* delta, const double* lambda, int32_t nref, const double* r,
                                            const double* v, double j_bound, const mpct_opts* opts,
                                            const mpct_osc_params* params, int32_t nsel, const int32_t* fields,
                                            int32_t nlev, const double* levels, mpct_robust_result* base,
                                            const mpct_draw_stats_result* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Goal attainment: goal-attainment selection over a scored grid, on the device (goal_attain.hip; DESIGN.md
 * §23).  The discrete counterpart of the reference's fgoalattain call: for each of G goal / weight vectors,
 * the candidates of the [C][k] table that minimise the attainment factor
 *     gamma = max_j (F_j - goal_j) / w_j ,
 * where a weight of 0 makes objective j a hard constraint F_j <= goal_j.  mpct_rank_device's weighted sum
 * cannot reach a candidate on a non-convex part of the front, mpct_pareto's front is not a decision and
 * neither takes a specification ("overshoot at most 10 %"); this call does all three, and a sweep of weight
 * directions says which few candidates win for most of them (wins).
 *
 * costs is [C][k] row-major, mpct_pareto's table: 1 <= k <= MPCT_PARETO_MAX_OBJ, 0 <= C <= MPCT_PARETO_MAX_C.
 * goals and weights are [G][k] row-major, 0 <= G <= MPCT_GOAL_MAX_G; 0 <= n_best <= MPCT_GOAL_MAX_BEST.
 *
 * Goal vector g is VALID when every w_j is either 0 or a finite positive value whose rounded reciprocal
 * iw_j = 1.0 / w_j is finite (a subnormal weight whose reciprocal overflows is not), at least one w_j > 0,
 * every goal_j with w_j > 0 is finite, and every goal_j with w_j = 0 is not NaN (+INFINITY there: no
 * constraint).  Negative weights (fgoalattain's over-attainment) are not supported: such a g is invalid.
 *
 * For a valid g and a candidate c:
 *   c is VALID by mpct_pareto's rule: none of its k costs is NaN; +-INFINITY are ordinary values.
 *   Hard objectives (w_j = 0): c must satisfy F_cj <= goal_j for each of them.
 *   Soft objectives (w_j > 0), in ascending j: d = F_cj - goal_j, rounded; term = d * iw_j, rounded -- two
 *   IEEE double operations, never a fused multiply-add, and iw_j the one correctly rounded division above.
 *   gamma starts at -INFINITY and active at the first soft j; whenever term > gamma, gamma = term and
 *   active = j.  So active is the SMALLEST j that attains the maximum.
 *   c is FEASIBLE for g when it is valid, passes every hard objective and has no NaN term.  (With a valid g
 *   a valid c has none: a soft goal is finite and 0 < iw_j < INFINITY.)  A feasible gamma may be +-INFINITY.
 *   Order among the feasible candidates: ascending gamma by `<`, so -0.0 equals +0.0; ties by ascending
 *   candidate index.  This is a total order, and it is what makes every result independent of the launch
 *   geometry: the candidate range is split into chunks whose partial lists and integer counts are merged, and
 *   neither the minimum of a total order nor an integer sum depends on the split.
 *
 *   best[g][0 .. n)     the first n = min(n_best, n_feasible[g]) candidates in that order
 *   gamma[g][0 .. n)    their attainment factors, as computed (a -0.0 stays -0.0)
 *   active[g][0 .. n)   their active objectives
 *                       the entries n .. n_best of the three rows are -1 / NaN / -1
 *   n_feasible[g]       the number of feasible candidates
 *   n_attained[g]       the number of feasible candidates with gamma <= 0 (every goal met)
 *   wins[c]             the number of g with best[g][0] == c; the call sets it to zero first
 * An INVALID g writes -1 / NaN / -1 to its rows and -1 to both counts and adds nothing to wins.
 * Any of the six pointers may be NULL, not all of them.  gamma or active needs n_best >= 1, neither needs
 * best; n_best = 0 with the counts or wins alone is fine.  A repeated call is bitwise identical; permuting the
 * goal vectors permutes the rows and counts and leaves wins unchanged.
 *
 * Argument errors, in this order and before any device is touched:
 *   MPCT_EINVAL  k < 1 or k > MPCT_PARETO_MAX_OBJ
 *   MPCT_EINVAL  C < 0 or G < 0
 *   MPCT_ERANGE  C > MPCT_PARETO_MAX_C or G > MPCT_GOAL_MAX_G
 *   MPCT_EINVAL  n_best < 0
 *   MPCT_ERANGE  n_best > MPCT_GOAL_MAX_BEST
 *   MPCT_EINVAL  costs NULL (with C > 0)
 *   MPCT_EINVAL  goals or weights NULL (with G > 0)
 *   MPCT_EINVAL  out NULL, or all six of its pointers NULL
 *   MPCT_EINVAL  best, gamma or active non-NULL with n_best = 0
 *   MPCT_EINVAL  mpct_goal_attain only: an invalid goal vector; the message names its row.  The device entry
 *                cannot read the arrays and applies the invalid-g rule above instead.
 * G = 0 returns MPCT_OK with wins zeroed (where given).  C = 0 is legal: every count of a valid g is 0 and
 * the rows are padded. */
#define MPCT_GOAL_MAX_G 1048576
#define MPCT_GOAL_MAX_BEST 16
typedef struct mpct_goal_result {
  int32_t* best;       /* [G][n_best] */
  double* gamma;       /* [G][n_best] */
  int32_t* active;     /* [G][n_best] */
  int32_t* n_feasible; /* [G] */
  int32_t* n_attained; /* [G] */
  int32_t* wins;       /* [C] */
} mpct_goal_result;

/* All pointers DEVICE pointers; enqueued on `stream` (NULL = default stream) and NOT synchronised.  Scratch
 * comes from hipMallocAsync / hipFreeAsync on that stream, as in mpct_pareto_device, so calls on different
 * streams are independent.  The work is bounded by C, G, k and n_best alone. */
int32_t mpct_goal_attain_device(const double* costs, int64_t C, int32_t k, const double* goals,
                                const double* weights, int64_t G, int32_t n_best, const mpct_goal_result* out,
                                void* stream);

/* Host pointers (MATLAB and C callers); needs no scenario.  device: HIP ordinal, -1 = the current device
 * (an ordinal out of range is MPCT_EINVAL).  Stages on a stream of its own and waits for that stream only,
 * as mpct_pareto does; the calling thread's current device is unchanged on return.  G = 0 and C = 0 need no
 * device.  Without a device: MPCT_EDEVICE with a message.  An argument error, a missing device and a device
 * ordinal out of range leave every output buffer, wins included, as it was. */
int32_t mpct_goal_attain(const double* costs, int64_t C, int32_t k, const double* goals, const double* weights,
                         int64_t G, int32_t n_best, int32_t device, const mpct_goal_result* out);

/* ---------------------------------------------------------------------------------------------
 * Trajectory envelopes over plant draws, on the device (envelope.hip).  The robust entries
 * reduce a candidate's D draws to numbers; these return what the loop did over time, across the draws: per
 * candidate, row and sample the band the signal stays in, its mean, its quantile lines and the draw that sits
 * on the edge -- the figure a Monte-Carlo study draws with `hold on` -- without C*D trajectories leaving the
 * device, and per candidate and row how wide that band is.
 *
 * Trajectories in mpct_result's layout, y[S][my][nit] and u[S][nu][nit] with simulation s = c*D + k.  Read as
 * it lies in memory, y is the table x[C][D][m] of mpct_draw_stats with m = my*nit (u: m = nu*nit), x_type
 * MPCT_STAT_F64, and the ENVELOPE of a side IS mpct_draw_stats of that table: alive is [C][D] or NULL, draw k
 * survives at sample (c, row, t) when it is alive and its value there is finite, and every field of
 * mpct_draw_stats_result is defined exactly as there -- n, mean (one accumulator from 0.0 over the survivors
 * in ascending k, divided by (double)n), lo / hi with the lowest draw that holds them and that draw's bits
 * (-0.0 == +0.0), the type-1 quantile, q_draw and cvar per level; n = 0 gives NaN / -1.  The arrays are
 * [C][rows][nit] and [C][rows][nit][nlev].  The envelope covers every sample, 0 .. nit-1.
 *
 * The spread of a side, per (c, row), element c*rows + row, over the samples t = t0 .. nit-1:
 *   spread        sum_t d(t), d(t) = hi(t) - lo(t) rounded once, in the fixed order of the performance indices:
 *                 lane (t - t0) mod 64 accumulates its d in ascending t from 0.0, then the 64 partials are
 *                 combined as a pairwise tree in lane order
 *   spread_max    max_t d(t);  t_spread_max  the first t that attains it
 * A row with n(t) = 0 at any t in the range gives NaN, NaN, -1.  The spread reads the lo and hi of its side
 * that the same call has just written, so those two pointers must be given with it.
 *
 * Any pointer of the two mpct_draw_stats_result and the two mpct_envelope_spread may be NULL, and each of the
 * four structs itself; a side without a result pointer is not read (its trajectory pointer may be NULL).
 * levels is a HOST pointer in every entry; nlev may be 0.  A repeated call is bitwise identical and a record
 * depends neither on C nor on the candidate's place in the batch.  Two kernels serve the levels, one lane per
 * column up to a draw count fixed by measurement and mpct_draw_stats' kernel above it; both implement the
 * one contract and give the same bits.
 *
 * Argument errors of mpct_envelope_device and mpct_envelope, in this order and before any device is touched:
 *   MPCT_EINVAL  C < 0, D < 1, my < 0, nu < 0 or nit < 1
 *   MPCT_EINVAL  t0 < 0 or t0 >= nit
 *   MPCT_EINVAL  nlev < 0 or nlev > MPCT_TAIL_MAX_LEVELS; nlev > 0 with levels NULL; a level that is NaN, <= 0 or > 1
 *   MPCT_EINVAL  a spread pointer of a side whose lo or hi is NULL
 *   MPCT_EINVAL  no result pointer at all in out_y and out_u
 *   MPCT_EINVAL  a quantile, cvar or q_draw pointer with nlev = 0
 *   MPCT_EINVAL  a result pointer in out_y with my < 1 or (C > 0) y NULL; the same for out_u, nu and u
 *   MPCT_ERANGE  D > MPCT_TAIL_MAX_DRAWS with nlev > 0
 *   MPCT_ERANGE  C*my*nit or C*nu*nit > MPCT_INDEX_MAX_ROWS
 * C = 0 is MPCT_OK and writes nothing. */
typedef struct mpct_envelope_spread {
  double* spread;        /* [C*rows] */
  double* spread_max;    /* [C*rows] */
  int32_t* t_spread_max; /* [C*rows] */
} mpct_envelope_spread;

/* All pointers DEVICE pointers (levels excepted); enqueued on `stream` (NULL = default stream) and NOT
 * synchronised.  Needs no scenario and no scratch: at most two kernel launches per side. */
int32_t mpct_envelope_device(const double* y, const double* u, const int32_t* alive, int64_t C, int32_t D, int32_t my,
                             int32_t nu, int32_t nit, int32_t t0, int32_t nlev, const double* levels,
                             const mpct_draw_stats_result* out_y, const mpct_draw_stats_result* out_u,
                             const mpct_envelope_spread* spread_y, const mpct_envelope_spread* spread_u, void* stream);

/* Host pointers (MATLAB and C callers), for trajectories from any source.  device: HIP ordinal, -1 = the
 * current device (an ordinal out of range is MPCT_EINVAL).  Stages on a stream of its own and waits for that
 * stream only; the calling thread's current device is unchanged on return.  Without a device: MPCT_EDEVICE
 * with a message. */
int32_t mpct_envelope(const double* y, const double* u, const int32_t* alive, int64_t C, int32_t D, int32_t my, int32_t nu,
                      int32_t nit, int32_t t0, int32_t nlev, const double* levels, int32_t device,
                      const mpct_draw_stats_result* out_y, const mpct_draw_stats_result* out_u,
                      const mpct_envelope_spread* spread_y, const mpct_envelope_spread* spread_u);

/* Score C candidates x D = nref draws and return the envelopes of their closed loops (host pointers; arguments
 * as mpct_eval_robust).  Per chunk of whole candidates (the chunking of mpct_eval_indices,
 * MPCT_INDEX_SCRATCH_BYTES of trajectory scratch) the closed loops run with their trajectories, J1 and status
 * written to scratch of the scenario's context; a classify kernel writes alive[c][k] by the rule of
 * mpct_eval_robust (status 0, J = sum_i J1_i finite, summed over i = 0 .. my-1 in that order, J <= j_bound with
 * 0 = 1e100; a candidate carrying MPCT_ST_SKIPPED or MPCT_ST_BADHORIZON on any draw has no live draw); and the
 * envelope kernels reduce the chunk's trajectories there.  Every record is bitwise independent of the chunk size.
 *   base     optional: mean and worst of J1, n_failed, worst_draw and status exactly as mpct_eval_robust
 *            defines them, from the same launch.  base->J1 must be NULL: the sample lives per chunk.
 *   opts     open_loop = 1 is MPCT_EINVAL; want_traj is ignored (the call sets it).
 * Errors, in this order and before any device is touched.  MPCT_EINVAL: s NULL; open_loop set; nref < 1; a
 * negative or NaN j_bound; t0 < 0 or t0 >= nit; nlev < 0 or > MPCT_TAIL_MAX_LEVELS, nlev > 0 with levels NULL, a
 * level that is NaN, <= 0 or > 1; a spread pointer of a side whose lo or hi is NULL; no result pointer at all
 * in base, out_y and out_u; base->J1 set; a quantile / cvar / q_draw pointer with nlev = 0; then everything
 * mpct_eval_batch rejects.  Then MPCT_ERANGE for nref > MPCT_TAIL_MAX_DRAWS with nlev > 0, and for C*my*nit or
 * C*nu*nit > MPCT_INDEX_MAX_ROWS.  C = 0 is MPCT_OK and writes nothing.  Without a device: MPCT_EDEVICE with a
 * message. */
int32_t mpct_eval_robust_envelope(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu, const double* delta,
                                  const double* lambda, int32_t nref, const double* r, const double* v, double j_bound,
                                  const mpct_opts* opts, int32_t t0, int32_t nlev, const double* levels,
                                  mpct_robust_result* base, const mpct_draw_stats_result* out_y,
                                  const mpct_draw_stats_result* out_u, const mpct_envelope_spread* spread_y,
                                  const mpct_envelope_spread* spread_u);

/* Same, all pointers DEVICE pointers except levels, enqueued on `stream` (NULL = default stream) and NOT
 * synchronised: the contract of mpct_eval_robust_indices_device, whose scratch and stream-ordering rule it
 * shares. */
int32_t mpct_eval_robust_envelope_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                         const double* delta, const double* lambda, int32_t nref, const double* r,
                                         const double* v, double j_bound, const mpct_opts* opts, int32_t t0, int32_t nlev,
                                         const double* levels, mpct_robust_result* base,
                                         const mpct_draw_stats_result* out_y, const mpct_draw_stats_result* out_u,
                                         const mpct_envelope_spread* spread_y, const mpct_envelope_spread* spread_u,
                                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCT_H */
