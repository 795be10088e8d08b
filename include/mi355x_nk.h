/* mi355x_nk.h — C ABI of libmi355x_nk.so: a MI355X (gfx950) Newton–Krylov inner loop that
 * drops in behind SciML/NonlinearSolve.jl's first-order step path.
 *
 * Every entry point replaces one seam of the reference (paths relative to the reference tree):
 *
 *   seam 1  linsolve backend   lib/NonlinearSolveBase/ext/NonlinearSolveBaseLinearSolveExt.jl:16-32
 *                              (LinearSolveJLCache functor → solve!(lincache)), tolerances pushed by
 *                              lib/NonlinearSolveFirstOrder/src/eisenstat_walker.jl:50,77
 *                              → nk_gmres_*                                     (GMRES(m) on device)
 *   seam 2  jac/jvp/vjp        lib/SciMLJacobianOperators/src/SciMLJacobianOperators.jl:167-182,238-243
 *                              (mul!(Jv, StatefulJacobianOperator, v)), f.jac at
 *                              lib/NonlinearSolveBase/src/jacobian.jl:237-258
 *                              → nk_residual / nk_jvp / nk_vjp / nk_jac_values / nk_spmv / nk_spmv_t
 *   seam 3  whole solver       ext/NonlinearSolvePETScExt.jl:38-167 pattern (SciMLBase.__solve) over
 *                              lib/NonlinearSolveFirstOrder/src/solve.jl:140-301 (init), :325-465 (step!)
 *                              lib/NonlinearSolveBase/src/solve.jl:360-387 (run to completion)
 *                              → nk_solver_init / _step / _solve / _reinit
 *
 * Conventions: C linkage, plain pointers and sizes, no C++ or torch types. All floating point data is
 * IEEE binary64. Every function returns an nk_status (0 = ok, <0 = error); the message of the last error
 * is available from nk_last_error(). Numerical non-convergence is a *retcode*, never an error status.
 * Vector arguments carry an explicit memory space (NK_HOST / NK_DEVICE). Host arrays are only read or
 * written during the call; device arrays must live on the context's device. Calls are asynchronous on the
 * context's HIP stream unless documented otherwise (anything returning scalars to the host synchronises).
 * A context is single-threaded. There is NO CPU fallback: without a HIP device nk_ctx_create fails.
 */
#ifndef MI355X_NK_H
#define MI355X_NK_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NK_VERSION_MAJOR 0
#define NK_VERSION_MINOR 1

/* ---------------------------------------------------------------- status / enums */
typedef enum {
  NK_OK = 0,
  NK_E_INVALID = -1,   /* bad argument */
  NK_E_HIP = -2,       /* HIP runtime error (no device, launch failure, ...) */
  NK_E_RCCL = -3,      /* RCCL error or librccl not loadable */
  NK_E_NOMEM = -4,
  NK_E_UNSUPPORTED = -5,
  NK_E_CALLBACK = -6,  /* a user callback returned non-zero */
  NK_E_SINGULAR = -7,  /* a preconditioner could not be built: zero / non-finite diagonal entry or ILU(0) pivot */
  NK_E_COMM = -8       /* a peer-mapped collective timed out (a rank stalled or died): results of this call are not valid */
} nk_status;

typedef enum { NK_HOST = 0, NK_DEVICE = 1 } nk_memspace;

/* SciMLBase.ReturnCode values that the first-order path can produce
 * (lib/NonlinearSolveFirstOrder/src/solve.jl:370,399,432; lib/NonlinearSolveBase/src/solve.jl:372-376,851;
 *  lib/NonlinearSolveBase/src/termination_conditions.jl:262,270,283,303,332). */
typedef enum {
  NK_RET_DEFAULT = 0,
  NK_RET_SUCCESS = 1,
  NK_RET_MAXITERS = 2,
  NK_RET_UNSTABLE = 3,
  NK_RET_STALLED = 4,
  NK_RET_INTERNAL_LINEAR_SOLVE_FAILED = 5,
  NK_RET_SHRINK_THRESHOLD_EXCEEDED = 6,
  NK_RET_MAXTIME = 7,
  NK_RET_FAILURE = 8,
  NK_RET_INTERNAL_LINESEARCH_FAILED = 9,
  NK_RET_CONVERGENCE_FAILURE = 10   /* NK_ALG_LIMITED_MEMORY_BROYDEN, NK_ALG_BROYDEN, NK_ALG_KLEMENT: the reset count reached max_resets (QuasiNewton/src/solve.jl:342-348) */
} nk_retcode;

typedef enum {
  NK_PROBLEM_QUADRATIC = 1,     /* f(u,p) = u.*u .- p          common/common_rootfind_testing.jl:15-17 */
  NK_PROBLEM_BRATU2D = 2,       /* 5-point Bratu (not in the reference)                  */
  NK_PROBLEM_BRUSSELATOR2D = 3, /* lib/NonlinearSolveFirstOrder/test/sparsity_tests__item1.jl:13-36     */
  NK_PROBLEM_USER = 100         /* user callbacks (f, jvp, vjp, jac) — NonlinearFunction fields         */
} nk_problem_kind;

/* NK_ALG_GAUSS_NEWTON: NewtonDescent in NORMAL FORM, JᵀJ δ = Jᵀ f through the normal-form operator — what GaussNewton
 * (lib/NonlinearSolveFirstOrder/src/gauss_newton.jl:11-23) does on a NonlinearLeastSquaresProblem with a Krylov linsolve
 * (descent/newton.jl:58-95,107-118; StatefulJacobianNormalFormOperator, SciMLJacobianOperators.jl:252-291). */
/* NK_ALG_LEVENBERG_MARQUARDT: the damped normal equations (JᵀJ + λDᵀD) δ = Jᵀ f through the same normal-form operator
 * plus a diagonal (DampedNewtonDescent in :normal_form mode, descent/damped_newton.jl:186-200,297-313 — the mode a Krylov
 * `linsolve` selects), geodesic acceleration (descent/geodesic_acceleration.jl:98-136) and the damping-based trust region
 * (levenberg_marquardt.jl:159-168,247-268). Needs a concrete J (concrete_jac = Val(true)) and a Krylov linsolve. */
/* NK_ALG_PSEUDO_TRANSIENT: DampedNewtonDescent with SwitchedEvolutionRelaxation damping in :simple mode
 * (descent/damped_newton.jl:283-288): the Newton step on J + α⁻¹ I — the shift is added to the diagonal of the concrete J
 * (`dampen_jacobian!!`) or to the matrix-free operator. */
/* NK_ALG_LIMITED_MEMORY_BROYDEN: LimitedMemoryBroyden without a line search (lib/NonlinearSolveQuasiNewton/src/lbroyden.jl): the
 * inverse Jacobian is a·I + U Vᵀ with `lb_threshold` columns, good-Broyden updates, NoChangeInStateReset(nsteps = 3). Needs
 * only the residual: no Jacobian, no JVP, no linear solve — nk_options.linsolve, the Krylov, forcing, preconditioner and
 * line-search fields are not read (linesearch != 0 is NK_E_INVALID: the line-search form is not built). One rank. */
/* NK_ALG_DFSANE: DFSane (lib/NonlinearSolveSpectralMethods: GeneralizedDFSane with the RobustNonMonotone line search): the step
 * is −ασ f with the spectral coefficient σ = ⟨δu,δu⟩/⟨δu,δf⟩. Needs only the residual, like algorithm 5: no Jacobian, no linear
 * solve; nk_options.linesearch != 0 (the search is part of the method), a forcing term or more than one rank are NK_E_INVALID.
 * A failed line search ends the solve with NK_RET_INTERNAL_LINESEARCH_FAILED. recompute_jacobian is ignored. */
/* NK_ALG_BROYDEN: Broyden without a line search (lib/NonlinearSolveQuasiNewton/src/broyden.jl) with init_jacobian = identity: the
 * inverse Jacobian is a dense n×n matrix on the device (nk_options.broyden_update_rule: good or bad Broyden), allocated by the
 * first step, or its diagonal (DiagonalStructure); NoChangeInStateReset(nsteps = 3). Needs only the residual, like algorithm 5:
 * the Krylov, forcing and preconditioner fields are not read; linesearch != 0 or more than one rank are NK_E_INVALID. A dense
 * structure with n above NK_BROYDEN_MAX_N is NK_E_UNSUPPORTED at init, before anything is allocated. */
/* NK_ALG_KLEMENT: Klement (klement.jl) with init_jacobian = identity: J is the vector α·1 (DiagonalStructure, not inverted), the
 * step is −fu ./ J, the reset test is IllConditionedJacobianReset (any(iszero, J)). The same restrictions as algorithm 7. */
typedef enum { NK_ALG_NEWTON_RAPHSON = 0, NK_ALG_TRUST_REGION = 1, NK_ALG_GAUSS_NEWTON = 2,
               NK_ALG_LEVENBERG_MARQUARDT = 3, NK_ALG_PSEUDO_TRANSIENT = 4, NK_ALG_LIMITED_MEMORY_BROYDEN = 5,
               NK_ALG_DFSANE = 6, NK_ALG_BROYDEN = 7, NK_ALG_KLEMENT = 8 } nk_algorithm;
#define NK_BROYDEN_MAX_N 32768   /* the dense inverse Jacobian of NK_ALG_BROYDEN at this size is 8 GiB */
/* nk_options.broyden_update_rule (broyden.jl:26-32); init_jacobian = true_jacobian is not built: NK_E_UNSUPPORTED */
typedef enum { NK_BROYDEN_GOOD = 0, NK_BROYDEN_BAD = 1, NK_BROYDEN_DIAGONAL = 2, NK_BROYDEN_TRUE_JACOBIAN = 16 } nk_broyden_rule;

/* which operator the Krylov solver sees as A (lib/NonlinearSolveBase/src/jacobian.jl:43-47,90-102) */
typedef enum {
  NK_LINSOLVE_GMRES_MATFREE = 0, /* StatefulJacobianOperator: fused device JVP                       */
  NK_LINSOLVE_GMRES_CSR = 1,     /* concrete sparse J (values refilled every step) + CSR SpMV        */
  NK_LINSOLVE_BANDED_LU = 2      /* concrete J, direct banded LU on device (config C2)                */
} nk_linsolve;

typedef enum {
  NK_ORTHO_MGS = 0,  /* modified Gram–Schmidt: the structure Krylov.jl's gmres uses [EXT]            */
  NK_ORTHO_CGS2 = 1, /* classical GS, always re-orthogonalised (2 fused passes)                       */
  NK_ORTHO_CGS = 2,  /* classical GS, re-orthogonalise only when ‖w'‖ < ‖w‖/√2 (DGKS)                 */
  NK_ORTHO_DCGS2 = 3, /* the default: CGS2 arithmetic with delayed re-orthogonalisation — two sweeps over the basis and
                       * (with the built-in linear operators) ONE reduction / all-reduce per Arnoldi step; operators
                       * reached through callbacks keep two reductions (and plain CGS2 when restart > 31)            */
  NK_ORTHO_DCGS2_1R = 4, /* insist on the one-reduction form (the pending vector's second projection and the new vector's
                       * first projection share a fused dot sweep; the Hessenberg column and the stopping test lag
                       * one step); falls back like NK_ORTHO_DCGS2 where the operator does not allow it            */
  NK_ORTHO_SSTEP = 5    /* s-step (communication-avoiding) Arnoldi: s operator applications build a block of basis vectors
                       * (A − θ_j I)…(A − θ_0 I) v — Newton basis with Leja-ordered Chebyshev shifts when real bounds of the
                       * operator's spectrum are known (Gershgorin discs of a CSR operator, the Bratu stencil's closed form,
                       * nk_gmres_set_spectrum_interval), monomial (θ = 0) otherwise — which is orthogonalised against the
                       * basis and within itself by block CGS in Pythagorean form, twice: three sweeps over the basis per
                       * s columns instead of two per column; the Gram blocks run on the FP64 matrix cores. Block size:
                       * nk_options.gmres_sstep / nk_gmres_set_block_size (0 = automatic: 15 Newton, 6 monomial). A block
                       * that loses rank numerically (Cholesky breakdown) finishes that solve with NK_ORTHO_DCGS2.           */
} nk_ortho;

/* basis of an s-step block (nk_options.gmres_sstep_basis / nk_gmres_set_sstep_basis) */
typedef enum {
  NK_SS_BASIS_AUTO = 0,     /* Newton where spectrum bounds are known, else monomial */
  NK_SS_BASIS_MONOMIAL = 1, /* A^j v (block size ≤ 8 advisable: κ grows like ρ^s)     */
  NK_SS_BASIS_NEWTON = 2    /* insist on the Newton basis (error if no bounds known)  */
} nk_ss_basis;

typedef enum { NK_FORCING_NONE = 0, NK_FORCING_EISENSTAT_WALKER2 = 1 } nk_forcing;

/* RadiusUpdateSchemes — lib/NonlinearSolveFirstOrder/src/trust_region.jl:59-147 */
typedef enum {
  NK_RUS_SIMPLE = 0, NK_RUS_NLSOLVE = 1, NK_RUS_NOCEDAL_WRIGHT = 2, NK_RUS_HEI = 3,
  NK_RUS_YUAN = 4, NK_RUS_BASTIN = 5, NK_RUS_FAN = 6
} nk_radius_update_scheme;

typedef enum { NK_COMM_NONE = 0, NK_COMM_RCCL = 1, NK_COMM_CALLBACKS = 2 } nk_comm_kind;

/* the nine SciMLBase termination modes (common/common_rootfind_testing.jl:3-13;
 * lib/NonlinearSolveBase/src/termination_conditions.jl:243-376). 0 is the reference's default (:385-389). */
typedef enum {
  NK_TM_ABSNORM_SAFEBEST = 0, NK_TM_NORM = 1, NK_TM_REL = 2, NK_TM_RELNORM = 3, NK_TM_RELNORM_SAFE = 4,
  NK_TM_RELNORM_SAFEBEST = 5, NK_TM_ABS = 6, NK_TM_ABSNORM = 7, NK_TM_ABSNORM_SAFE = 8
} nk_termination_mode;

/* ---------------------------------------------------------------- opaque handles */
typedef struct nk_ctx nk_ctx;         /* device, stream, communicator, scratch                     */
typedef struct nk_csr nk_csr;         /* row-partitioned CSR (f64 values, i32 indices) + halo plan */
typedef struct nk_problem nk_problem; /* residual / JVP / VJP / Jacobian provider                  */
typedef struct nk_gmres nk_gmres;     /* GMRES(m) workspace (LinearSolve "LinearCache" analogue)    */
typedef struct nk_solver nk_solver;   /* GeneralizedFirstOrderAlgorithmCache analogue               */
typedef struct nk_bandlu nk_lu;       /* banded LU factorisation (LinearSolve factorisation-cache analogue) */
typedef struct nk_batch nk_batch;     /* ensemble of small dense systems, one per GPU thread */

/* ---------------------------------------------------------------- plain structs */

/* NLStats (nf, njacs, nfactors, nsolve, nsteps) — incremented where the reference increments them
 * (lib/NonlinearSolveBase/src/utils.jl:201, jacobian.jl:238, ext/...LinearSolveExt.jl:20,84,
 *  lib/NonlinearSolveBase/src/solve.jl:844) — extended with device-side work counters. */
typedef struct {
  int64_t nf, njacs, nfactors, nsolve, nsteps;
  int64_t gmres_iters;     /* total Arnoldi steps                        */
  int64_t op_applies;      /* SpMV / JVP / VJP applications              */
  int64_t allreduces;      /* collective calls issued                    */
  int64_t halo_exchanges;
} nk_stats;

typedef struct {
  int32_t iters;        /* Arnoldi steps performed                                    */
  int32_t restarts;     /* completed restart cycles                                   */
  int32_t converged;    /* 1: ‖r‖ ≤ atol + rtol‖r0‖ ; 0: iteration cap hit            */
  int32_t failed;       /* 1: non-finite residual (maps to ReturnCode.Failure)        */
  double  rnorm0;       /* ‖b − A x0‖₂ (‖Pl⁻¹(b − A x0)‖₂ with a left preconditioner) */
  double  rnorm;        /* last (recurrence) residual norm estimate                   */
} nk_gmres_info;

/* One row per nonlinear step: the TraceMinimal fields (lib/NonlinearSolveBase/src/tracing.jl:259-309)
 * plus the Krylov / forcing / trust-region scalars. */
typedef struct {
  int32_t iter;
  int32_t gmres_iters;
  int32_t accepted;      /* trust region: step accepted (always 1 for Newton) */
  int32_t reserved;
  double  fnorm_inf;     /* ‖f(u)‖∞ after the step                            */
  double  step_norm2;    /* ‖δu‖₂                                             */
  double  eta;           /* Krylov reltol used                                */
  double  trust_region;  /* Δ after the update                                */
  double  rho;
} nk_trace_entry;

typedef struct {
  /* --- algorithm (raphson.jl:30-43, trust_region.jl:25-43) */
  int32_t algorithm;            /* nk_algorithm                                                     */
  int32_t linsolve;             /* nk_linsolve                                                      */
  int32_t maxiters;             /* 1000  (FirstOrder/src/solve.jl:142)                              */
  int32_t termination_norm;     /* internalnorm of the termination mode: 0 = maximum∘abs (default), 1 = 2-norm */
  double  abstol;               /* ≤0 → 3.0e-13 (common_defaults.jl:44-48)                          */
  double  reltol;               /* ≤0 → 3.0e-13; only forwarded to the linear solver                */
  double  maxtime;              /* seconds, ≤0 → none (Base/src/solve.jl:846-856)                   */
  /* --- Krylov protocol */
  int32_t gmres_restart;        /* m; ≤0 → 30                                                       */
  int32_t gmres_maxiters;       /* inner-iteration cap per linear solve; ≤0 → 300                   */
  int32_t gmres_ortho;          /* nk_ortho                                                         */
  int32_t gmres_fixed_iters;    /* >0: run exactly this many Arnoldi steps (fixed-work protocol)    */
  double  lin_abstol;           /* <0 → forward the nonlinear abstol (FirstOrder/src/solve.jl:203)  */
  double  lin_reltol;           /* <0 → forward the nonlinear reltol                                */
  /* --- forcing (eisenstat_walker.jl:18-29) */
  int32_t forcing;              /* nk_forcing                                                       */
  int32_t ew_safeguard;         /* 1                                                                */
  double  ew_eta0, ew_eta_max, ew_gamma, ew_alpha, ew_safeguard_threshold; /* .5 .9 .9 2 .1         */
  /* --- trust region (trust_region.jl:25-33,320-384); 0 → the scheme's default */
  int32_t radius_update_scheme; /* nk_radius_update_scheme                                          */
  int32_t max_shrink_times;     /* 32                                                               */
  double  max_trust_radius, initial_trust_radius, step_threshold, shrink_threshold,
          expand_threshold, shrink_factor, expand_factor;
  /* --- termination: AbsNormSafeBestTerminationMode(maximum∘abs; max_stalled_steps = 32)
   *     (termination_conditions.jl:243-336,385-389); numeric defaults of the mode struct are [EXT] */
  int32_t patience_steps;       /* 100                                                              */
  int32_t max_stalled_steps;    /* 32; <0 disables the stall test                                   */
  double  patience_objective_multiplier; /* 3                                                        */
  double  min_max_factor;       /* 1.3                                                              */
  double  protective_threshold; /* ≤0 → off                                                         */
  /* --- tracing */
  int32_t store_trace;          /* keep nk_trace_entry rows (costs one extra 2-norm per step)       */
  int32_t termination_mode;     /* nk_termination_mode; 0 = AbsNormSafeBest, the reference default  */
  /* --- preconditioner of the Krylov solver (`precs`): 0 none, >0 Chebyshev polynomial of that degree, its
   *     interval re-estimated for every new Jacobian (lambda_max by power iteration, lambda_min = max/ratio) */
  int32_t cheb_degree;
  int32_t linesearch;           /* 0 none (missing), 1 BackTracking, 2 LineSearchesJL(Static), 3 LineSearchesJL(StrongWolfe),
                                   4 LineSearchesJL(MoreThuente), 5 LineSearchesJL(HagerZhang) [EXT: LineSearches.jl defaults] — globalisation
                                   Val(:LineSearch), lib/NonlinearSolveFirstOrder/src/solve.jl:392-408               */
  double  cheb_ratio;           /* ≤1 → 30 */
  /* --- BackTracking line search (LineSearch.jl / LineSearches.jl [EXT]: c_1 = 1e-4, ρ_hi = 0.5, ρ_lo = 0.1,
   *     order = 3, iterations = 1000) on ϕ(α) = ½‖f(u + α δu)‖², ϕ'(0) = fuᵀ J δu */
  double  ls_c1, ls_rho_hi, ls_rho_lo;
  int32_t ls_order;             /* 2 | 3 */
  int32_t ls_maxiters;
  /* --- built-in multigrid V-cycle as the Krylov right preconditioner (BRATU2D, BRUSSELATOR2D; compiled grid problems on one
   *     rank), re-linearised for every new Jacobian like `precs(A, p)`: mg_nu smoothing steps (0 = off), coarsest grid side
   *     ≤ mg_coarse (0 → the problem kind's default: nk_gmres_set_multigrid_preconditioner) */
  int32_t mg_nu;
  int32_t mg_coarse;
  /* --- concrete Jacobian of the built-in problems: 0 = closed-form values (what `f.jac` would supply), 1 = the
   *     colour-compressed assembly of `AutoSparse` + column colouring (ncolors seeded JVPs + decompression,
   *     lib/NonlinearSolveBase/src/jacobian.jl:244-247) every time the Jacobian is refreshed */
  int32_t jac_colored;
  /* --- LevenbergMarquardt (lib/NonlinearSolveFirstOrder/src/levenberg_marquardt.jl:37-64; constructor defaults in
   *     brackets): GeodesicAcceleration(DampedNewtonDescent(LM damping)) + LevenbergMarquardtTrustRegion */
  int32_t lm_disable_geodesic;          /* [0] 1 = plain damped Newton step (disable_geodesic = Val(true))           */
  double  lm_damping_initial;           /* [1]    λ₀                                                                  */
  double  lm_damping_increase_factor;   /* [2]    λ ← 2λ after a step that was not taken                              */
  double  lm_damping_decrease_factor;   /* [3]    λ ← λ/3 after an accepted step                                      */
  double  lm_min_damping_D;             /* [1e-8] floor of DᵀD = running max of diag(JᵀJ)                             */
  double  lm_alpha_geodesic;            /* [0.75] a step is taken only if 2‖a‖ ≤ α‖v‖                                 */
  double  lm_finite_diff_step_geodesic; /* [0.1]  h of the second directional derivative                              */
  double  lm_b_uphill;                  /* [1]    uphill moves: (1 − β)^b · ‖f_new‖ ≤ loss_old                        */
  /* --- PseudoTransient (lib/NonlinearSolveFirstOrder/src/pseudo_transient.jl:37-57): (J + α⁻¹ I) δ = f with switched
   *     evolution relaxation α⁻¹ ← α⁻¹·‖f‖₂/‖f_prev‖₂; mass matrix: identity, or a diagonal through
   *     nk_solver_set_mass_matrix_diagonal */
  double  pt_alpha_initial;             /* [1e-3] initial pseudo time step α                                          */
  int32_t gmres_sstep;                  /* [0]    NK_ORTHO_SSTEP: basis columns per block (1..16; 0 = automatic)      */
  int32_t gmres_sstep_basis;            /* [0]    nk_ss_basis                                                         */
  /* --- a built-in preconditioner object on the concrete J, rebuilt numerically for every new Jacobian like `precs(A, p)`
   *     (needs a concrete-J linsolve): 0 none, 1 Jacobi, 2 ILU(0) in the matrix's ordering, 3 ILU(0) multicolour,
   *     4 aggregation algebraic multigrid (nk_precond_create_amg with its defaults) */
  int32_t precond_kind;                 /* [0]                                                                        */
  int32_t precond_side;                 /* [1]    nk_side: the reference's tutorial precs return (Pl, I): left        */
  /* --- LimitedMemoryBroyden (lib/NonlinearSolveQuasiNewton/src/lbroyden.jl:20-35); a value <= 0 selects the default */
  int32_t lb_threshold;                 /* [10]   columns of U and V, 1..32 (more: NK_E_INVALID); clamped to maxiters          */
  int32_t lb_max_resets;                /* [3]    the reset that brings the count to this ends the solve (ConvergenceFailure) */
  double  lb_reset_tolerance;           /* [eps^(3/4)] NoChangeInStateReset's tolerance (reset_conditions.jl:34)              */
  double  lb_alpha;                     /* [nothing] J⁻¹ starts as I/alpha; default alpha = 2‖fu‖₂/max(‖u‖₂, 1), 1 if ‖fu‖₂ < 1e-5 */
  /* --- DFSane (lib/NonlinearSolveSpectralMethods/src/dfsane.jl:21-35); a value <= 0 selects the default */
  double  sane_sigma_min;               /* [1e-10] |σ| outside [sigma_min, sigma_max] is replaced by clamp(1/‖f‖₂, 1, 1e5)     */
  double  sane_sigma_max;               /* [1e10]                                                                              */
  double  sane_sigma_1;                 /* [0 = nothing] the first σ; nothing: ⟨u,u⟩/⟨u,f⟩ (then the bounds test). Any sign.   */
  int32_t sane_M;                       /* [10]   length of the merit history, 1..32 (more: NK_E_INVALID)                      */
  double  sane_gamma;                   /* [1e-4]                                                                              */
  double  sane_tau_min;                 /* [0.1]                                                                               */
  double  sane_tau_max;                 /* [0.5]                                                                               */
  int32_t sane_n_exp;                   /* [2]    merit ‖f‖₂^n_exp, 1 or 2 (else NK_E_INVALID)                                 */
  int32_t sane_max_inner_iterations;    /* [100]  (minus trial, plus trial) pairs of one line search before it has failed      */
  /* --- Broyden and Klement (lib/NonlinearSolveQuasiNewton/src/broyden.jl:34-49, klement.jl:29-48); a value <= 0 selects the default */
  int32_t broyden_update_rule;          /* [0]    nk_broyden_rule; + NK_BROYDEN_TRUE_JACOBIAN: init_jacobian = true_jacobian(_diagonal), NK_E_UNSUPPORTED */
  int32_t qn_max_resets;                /* [100]  the reset that brings the count to this ends the solve (ConvergenceFailure) */
  double  qn_reset_tolerance;           /* [eps^(3/4)] NoChangeInStateReset's tolerance (Broyden)                             */
  double  qn_alpha;                     /* [nothing] J starts as alpha·I; default alpha = 2‖fu‖₂/max(‖u‖₂, 1), 1 if ‖fu‖₂ < 1e-5 */
} nk_options;

/* in-place callbacks of a user problem: NonlinearFunction{true}(f!; jvp, vjp, jac)
 * (signatures pinned by lib/SciMLJacobianOperators/test/core_tests__item2.jl:38-40,62-67 and
 *  lib/NonlinearSolveFirstOrder/test/rootfind_tests__item20.jl:17-32). All pointers are DEVICE pointers
 *  of local length n; `stream` is the hipStream_t the work must be ordered on. Return 0 on success. */
typedef int (*nk_residual_fn)(void *user, const double *u, double *f, void *stream);
typedef int (*nk_jvp_fn)(void *user, const double *v, const double *u, double *Jv, void *stream);
typedef int (*nk_vjp_fn)(void *user, const double *v, const double *u, double *vJ, void *stream);
typedef int (*nk_jacvals_fn)(void *user, const double *u, double *csr_vals, void *stream);
typedef struct {
  nk_residual_fn residual; /* required */
  nk_jvp_fn jvp;           /* NULL ⇒ forward differences through `residual`, (f(u+εv) − f(u))/ε, ε = √eps — the
                            * AutoFiniteDiff pushforward of SciMLJacobianOperators.jl:396-414 */
  nk_vjp_fn vjp;           /* required for TrustRegion on the matrix-free path */
  nk_jacvals_fn jac_values;/* NULL ⇒ concrete-J linsolves assemble J on the pattern given at create from ncolors seeded
                            * JVPs + decompression (greedy column colouring, cached per pattern; jacobian.jl:244-247) */
} nk_user_callbacks;

/* generic operator for nk_gmres: y = A x on device (an AbstractSciMLOperator / FunctionOperator) */
typedef int (*nk_matvec_fn)(void *user, const double *x, double *y, void *stream);

/* communicator callbacks (used for gloo/CPU-side collectives in tests, or any host transport).
 * Buffers are DEVICE pointers; the callback must have completed the operation (device-visible) before
 * it returns, after synchronising `stream` itself if it needs the data on the host. */
typedef struct {
  int (*allreduce)(void *user, double *buf, int count, int op /*0 sum, 1 max*/, void *stream);
  /* exchange bytes with every peer: send_bytes[p] bytes at send+send_off[p] to peer p, receive likewise */
  int (*alltoallv)(void *user, const void *send, const int64_t *send_off, const int64_t *send_bytes,
                   void *recv, const int64_t *recv_off, const int64_t *recv_bytes, void *stream);
  void *user;
} nk_comm_callbacks;

/* ---------------------------------------------------------------- library / context */
const char *nk_version(void);
const char *nk_last_error(void);              /* thread-local; never NULL */
int nk_device_count(int *count);

/* device_id: HIP ordinal. stream: the hipStream_t to enqueue on (NULL = the default/null stream). */
int nk_ctx_create(int device_id, void *stream, nk_ctx **out);
int nk_ctx_destroy(nk_ctx *ctx);
int nk_ctx_set_stream(nk_ctx *ctx, void *stream);
int nk_ctx_synchronize(nk_ctx *ctx);
/* deterministic=1 (default): fixed-order two-stage reductions, bitwise reproducible run to run. */
int nk_ctx_set_deterministic(nk_ctx *ctx, int deterministic);
/* Multi-rank CSR SpMV: run the halo exchange on a second stream while the row blocks that read no halo column are
 * computed (off by default; also enabled by NK_HALO_OVERLAP=1 in the environment at context creation). */
int nk_ctx_set_halo_overlap(nk_ctx *ctx, int on);

/* Device buffers for host languages that have no GPU array type of their own (a Julia session without AMDGPU.jl, plain C):
 * with them every vector argument of the ABI can be passed with memspace = NK_DEVICE and stays resident between calls.
 * nk_device_copy kind: 0 host→device, 1 device→host, 2 device→device; ordered on the context's stream, complete on return. */
int nk_device_alloc(nk_ctx *ctx, int64_t bytes, void **out);
int nk_device_free(nk_ctx *ctx, void *ptr);
int nk_device_copy(nk_ctx *ctx, void *dst, const void *src, int64_t bytes, int kind);
/* In-place updates of resident vectors (DEVICE pointers, local length n) for host languages whose resident vector type is a
 * library buffer (Julia's DeviceVector): y = a x + b y and y = a — with nk_dot / nk_nrm2 / nk_norm_inf / nk_axpy below, what
 * `@bb axpy!`, `copyto!` and the termination norms of the reference's step! need (FirstOrder/src/solve.jl:403,438,460).
 * They follow the contract of the BLAS-1 building blocks stated at the end of this header; nk_vec_fill stores the bit pattern of
 * `a` in every element (so −0.0 stays −0.0 and a NaN keeps its payload). */
int nk_vec_axpby(nk_ctx *ctx, int64_t n, double a, const double *x, double b, double *y);
int nk_vec_fill(nk_ctx *ctx, int64_t n, double a, double *y);

/* Per-kernel-family timing (bench.py's roofline numbers). Off by default; when on, every launch of a profiled
 * family is issued with hipExtLaunchKernelGGL start/stop events, i.e. the kernel's own begin/end device
 * timestamps on the context's stream — the quantity rocprofv3's kernel trace reports. `launches` counts logical
 * operations (a multidot over 31 columns is one operation although it is two kernel launches). */
int nk_ctx_profile_enable(nk_ctx *ctx, int on);          /* on=1 also resets the accumulators */
int nk_ctx_profile_kernel_count(void);
int nk_ctx_profile_query(nk_ctx *ctx, int kernel_id, const char **name, int64_t *launches,
                         double *total_ms, double *total_algorithmic_bytes);

/* One process per GPU. Rank 0 creates an id, the host language broadcasts the 128 bytes
 * (torch.distributed / MPI.jl / Distributed.jl), every rank calls nk_ctx_comm_init_rccl. */
int nk_comm_unique_id(char id_out[128]);
int nk_ctx_comm_init_rccl(nk_ctx *ctx, int nranks, int rank, const char id[128]);
int nk_ctx_comm_init_callbacks(nk_ctx *ctx, int nranks, int rank, const nk_comm_callbacks *cb);
/* xGMI-native small collectives on top of either communicator (which keeps serving set-up and large exchanges): every
 * rank allocates an uncached arena on its GPU and exports it (hipIpcGetMemHandle, 64 bytes); the host language
 * all-gathers the handles; every rank maps all of them. Afterwards the Krylov all-reduces (≤ 128 doubles) and the halo
 * exchanges run as ONE small kernel each: a rank stores its partial sums / its halo entries straight into every peer's
 * arena, releases a sequence flag (system scope), polls the flags of its peers and combines in rank order — bitwise
 * reproducible, no RCCL launch (≈ 20 µs) on the critical path of an Arnoldi step.
 *   nk_ctx_comm_peer_handle : allocate the arena (arena_bytes ≤ 0: 64 MiB) and return its IPC handle
 *   nk_ctx_comm_enable_peer : handles = nranks × 64 bytes in rank order (this rank's own entry is ignored)
 *   nk_ctx_comm_peer_status : *enabled; *errors = time-outs seen by the device kernels (0 in a healthy run) */
#define NK_IPC_HANDLE_BYTES 64
int nk_ctx_comm_peer_handle(nk_ctx *ctx, int64_t arena_bytes, char handle_out[NK_IPC_HANDLE_BYTES]);
int nk_ctx_comm_enable_peer(nk_ctx *ctx, const char *handles);
int nk_ctx_comm_peer_status(nk_ctx *ctx, int *enabled, int64_t *errors);
/* the communicator's all-reduce on a DEVICE buffer, in place (op 0 = sum, 1 = max), through whatever transport the context
 * holds (peer-mapped arenas up to 512 values, RCCL, callbacks); blocking. For self-checks of a multi-GPU set-up
 * (tools/multi_gpu_selfcheck.py) and for host code that needs a global reduction of its own. */
int nk_ctx_comm_allreduce(nk_ctx *ctx, double *buf, int count, int op);
/* collective: a few all-reduces with known answers; if any rank sees a wrong value or a time-out the fast path is
 * switched off on every rank (*ok = 0) and the base transport serves all collectives */
int nk_ctx_comm_peer_selftest(nk_ctx *ctx, int *ok);
int nk_ctx_comm_peer_disable(nk_ctx *ctx);   /* before any problem / matrix was created on the context */
int nk_ctx_comm_info(nk_ctx *ctx, int *kind, int *nranks, int *rank);
/* *shared = 1 if several ranks of the communicator run on ONE device (found out collectively when the communicator was set up,
 * from the devices' PCI bus ids; NK_DEVICE_SHARED=0/1, set alike on every rank, overrides): such ranks do not use the one form that
 * needs a whole device per rank — the resident matrix-powers kernel on ranks. One process per GPU: 0.
 * nk_ctx_comm_init_rccl / nk_ctx_comm_init_callbacks are COLLECTIVE for this reason (one small all-reduce through the transport). */
int nk_ctx_comm_device_shared(nk_ctx *ctx, int *shared);

/* contiguous row-range partition used everywhere: rank r owns [r*n/P, (r+1)*n/P) rounded down to a
 * multiple of `granule` (a grid line for stencil problems). Pure host logic, no device needed. */
int nk_partition_range(int64_t n_global, int64_t granule, int nranks, int rank,
                       int64_t *row_begin, int64_t *row_end);

/* ---------------------------------------------------------------- sparse matrices */
/* Local rows [row_begin, row_begin+nrows_local) of a square n_global matrix, GLOBAL column ids.
 * index_bits 32|64, index_base 0|1 (Julia). Copies (and for nranks>1 builds the halo plan — collective).
 * vals may be NULL (pattern only; fill later with nk_csr_set_values / nk_jac_values). */
int nk_csr_create(nk_ctx *ctx, int64_t nrows_local, int64_t n_global, int64_t row_begin, int64_t nnz,
                  int index_bits, int index_base, const void *rowptr, const void *colind,
                  const double *vals, int memspace, nk_csr **out);
/* Julia's SparseMatrixCSC{Float64,Int} (colptr,rowval,nzval) of the WHOLE n × n matrix, as every rank holds it:
 * converts CSC→CSR once on the host and keeps this rank's row range (nk_partition_range with granule 1, or the
 * explicit range of the _rows form — whole grid lines for stencil problems). Collective on several ranks. */
int nk_csr_create_from_csc(nk_ctx *ctx, int64_t n, int64_t nnz, int index_bits, int index_base,
                           const void *colptr, const void *rowval, const double *nzval, nk_csr **out);
int nk_csr_create_from_csc_rows(nk_ctx *ctx, int64_t n, int64_t nnz, int index_bits, int index_base,
                                const void *colptr, const void *rowval, const double *nzval,
                                int64_t row_begin, int64_t nrows_local, nk_csr **out);
int nk_csr_destroy(nk_csr *A);
int nk_csr_set_values(nk_csr *A, const double *vals, int memspace);
/* New values for a matrix created by nk_csr_create_from_csc(_rows), given in the CSC order of that call (Julia:
 * `nonzeros(J)` of the SparseMatrixCSC `f.jac(J, u, p)` refreshes every Newton step): one gather on the device through the
 * permutation remembered at creation — no new conversion, no new pattern upload. nnz_csc = length of nzval. */
int nk_csr_set_values_csc(nk_csr *A, const double *nzval, int64_t nnz_csc, int memspace);
int nk_csr_get_values(nk_csr *A, double *vals, int memspace);
int nk_csr_info(nk_csr *A, int64_t *nrows_local, int64_t *n_global, int64_t *nnz, int64_t *n_halo);
/* Device pointer of the local values (nnz doubles). From this call on the library cannot see when the values change, so it
 * treats every value-dependent cache of this matrix as always stale: the transposed values are permuted again before every
 * nk_spmv_t, cached spectrum bounds are recomputed, the speculative Jacobian fill is off. */
double *nk_csr_values_device(nk_csr *A);
/* y = A x  (x, y local slices; halo exchanged internally).  nk_spmv_t: y = Aᵀ x (the contributions to entries other
 * ranks own return through the halo plan in reverse and are added in rank order: bitwise reproducible). */
int nk_spmv(nk_csr *A, const double *x, double *y, int memspace);
int nk_spmv_t(nk_csr *A, const double *x, double *y, int memspace);
/* Matrix powers — the s operator applications an s-step Arnoldi block makes back to back (the `mul!(Jv, A, v)` of
 * lib/SciMLJacobianOperators/src/SciMLJacobianOperators.jl:238-243, s times in a row on a concrete J):
 *   Y[:, p] = scale·(A Y[:, p−1] − θ_p Y[:, p−1]),  p = 0 … s−1,  Y[:, −1] = x   (theta: s host values, NULL = plain powers;
 * ldy ≥ local rows). A banded matrix small enough to be held in the chip's vector registers (≤ #CUs × 6144 rows, ≤ 5 / 8 / 16
 * entries per row, columns within ±1024 rows of their band; one rank) takes ONE launch that reads the matrix once
 * (*resident = 1, csrc/nk_powers.hip) — also a matrix made of two equal segments that is banded segment by segment (the
 * (i, j, species) ordering of a two-species system, docs/src/tutorials/large_systems.md) and / or whose bands close to a ring
 * (periodic boundaries); any other matrix takes s streaming SpMV launches. The columns are bit-identical either way.
 * NK_SPMV_POWERS=0 disables the resident kernel.
 * Device memory: a matrix that takes the plain band form keeps, for as long as it lives, a packed table of its pattern beside
 * rowptr / col (built once with the plan, never when values change; csrc/nk_pw_pack.h): 12 / 20 / 36 bytes per row of every band
 * at ≤ 5 / 8 / 16 entries per row — 12.6 MB for the 1024² Bratu Jacobian. A pattern the table's 16-bit fields cannot hold is
 * not eligible and keeps the streaming launches.
 * Several ranks: whether the resident kernel applies is decided ONCE per matrix by all ranks together — the first nk_csr_powers
 * or s-step linear solve on a row-partitioned matrix is COLLECTIVE (two small all-reduces through the communicator); every rank
 * must reach it, also a rank whose share would not qualify. */
int nk_csr_powers(nk_csr *A, const double *x, double *Y, int64_t ldy, int s, const double *theta, double scale, int memspace,
                  int *resident);
/* Which form of the resident kernel a CSR PATTERN (global column ids, one rank) fits on a device with num_cus compute units —
 * host arithmetic only, no device needed: layout[0] = 0 none (streaming launches), 1 plain bands, 2 segments and / or ring;
 * [1] slices of 1024 rows per band (and segment), [2] register slots per row (5 / 8 / 16), [3] bands (= workgroups),
 * [4] segments, [5] 1 = the bands of a segment close to a ring. (The device additionally needs all bands resident at once.) */
int nk_csr_powers_layout(int64_t nrows, const int32_t *rowptr, const int32_t *col, int num_cus, int layout[6]);
/* out_j = Σ_i A_ij² — diag(AᵀA), what LevenbergMarquardt's damping takes its DᵀD from (`sum!(abs2, J_diag_cache, J')`,
 * levenberg_marquardt.jl:133-148). Row-partitioned matrices: the same reverse halo exchange as nk_spmv_t. */
int nk_csr_colsumsq(nk_csr *A, double *out, int memspace);

/* ---------------------------------------------------------------- problems (seam 2) */
/* params: QUADRATIC {n, p}; BRATU2D {n_side, lambda, scale (0 → h², i.e. h²F)};
 *         BRUSSELATOR2D {N_g, A, B, alpha, dx}.  The problem partitions itself over the ctx's ranks.
 * Accepted sizes: BRATU2D 1 <= n_side < 2^30 (the JVP kernel indexes a grid line with an int; anything else, NaN included, is
 * NK_E_INVALID with a message), and n_side >= the number of ranks; BRUSSELATOR2D N_g >= 3. */
int nk_problem_create(nk_ctx *ctx, int kind, const double *params, int nparams, nk_problem **out);
/* csr pattern (local rows, global columns, 0-based int32/int64) is optional: NULL ⇒ no concrete J. */
int nk_problem_create_user(nk_ctx *ctx, int64_t n_local, int64_t n_global, int64_t row_begin,
                           const nk_user_callbacks *cb, void *user, nk_csr *jac_pattern,
                           nk_problem **out);
int nk_problem_destroy(nk_problem *P);
int nk_problem_size(nk_problem *P, int64_t *n_local, int64_t *n_global, int64_t *row_begin);
int nk_problem_set_params(nk_problem *P, const double *params, int nparams);  /* reinit!(cache; p) */
int nk_problem_initial_guess(nk_problem *P, double *u0, int memspace);
int nk_residual(nk_problem *P, const double *u, double *f, int memspace);
int nk_jvp(nk_problem *P, const double *u, const double *v, double *Jv, int memspace);
int nk_vjp(nk_problem *P, const double *u, const double *v, double *vJ, int memspace);
/* concrete sparse Jacobian: pattern once, closed-form values per call (f.jac(J,u,p), jacobian.jl:241) */
int nk_problem_jac_csr(nk_problem *P, nk_csr **out);
int nk_jac_values(nk_problem *P, const double *u, int memspace, nk_csr *J);
/* colour-compressed assembly: ncolors JVPs with seed vectors + decompression — the structure of
 * DI.jacobian! with AutoSparse (jacobian.jl:244-247; colouring ext/...SparseMatrixColoringsExt.jl:13-28) */
int nk_jac_values_colored(nk_problem *P, const double *u, int memspace, nk_csr *J, int *ncolors);

/* ---------------------------------------------------------------- compiled grid problems (kernel generation, full size)
 * A residual given pointwise on a 2-D grid through a radius-1 stencil: what the reference's user writes as `f` and lets
 * SciMLJacobianOperators differentiate with forward-mode duals (J·v) and sparse AD fill into `jac_prototype`. `source` is HIP C++
 * defining
 *     template <typename T> __device__ void nk_point(const nk_nbhd<T> &u, const nk_real *p, nk_site s, T *f);
 * with  u(di, dj, c = 0)  component c at node (i + di, j + dj), di, dj ∈ {−1, 0, 1} (write them as constants). An offset
 *                         that is no point of the stencil returns NaN — a corner (di != 0 && dj != 0) with NK_GRID_STAR,
 *                         anything two nodes away with either stencil — so a wrong source shows at the first residual;
 *       s                 {i, j, nx, ny}: the node and the grid;
 *       p                 nparams doubles, 0..32 (nk_problem_set_params replaces them);
 *       f                 receives the node's dof residuals (entries the source does not write are zero);
 *       nk_real           double — there is no Float32 mode.
 * It is compiled at run time (hiprtc, gfx950, -O3 -ffp-contract=off -std=c++17) behind the dual-number prelude of the ensemble
 * kernels (the same operators and elementary functions as for nk_f) into three kernels, one grid node per thread: the residual
 * (T = double), the exact J·v (T = a dual with one partial: value from u, partial from v) and the values of J on the stencil's
 * CSR pattern (a dual with npts·dof partials, unit seeds). No finite differences anywhere.
 * Geometry: nx × ny nodes, nx, ny >= 3 (not necessarily square); dof = 1..4 components per node; stencil NK_GRID_STAR (5 points)
 * or NK_GRID_BOX (9 points, dof <= 2: a row has at most 20 partials); boundary NK_GRID_DIRICHLET0 (a neighbour outside the grid
 * reads as the constant 0 and has no column), NK_GRID_PERIODIC (indices wrap in both directions) or a kind per side packed by
 * NK_GRID_SIDES (mirror walls, a channel: see the enum below). Unknown c of node (i, j) is
 * element c·nx·ny + j·nx + i (the Brusselator's layout). Several ranks: "Several ranks" below.
 * The object is an nk_problem of kind NK_PROBLEM_USER whose callbacks launch the generated kernels: every algorithm, linear
 * solver and preconditioner object takes it as it takes any callback problem — so the matrix-free GMRES keeps the callback
 * kind's two reductions per Arnoldi step and unfused output scale, and Jᵀv (TrustRegion, normal forms) is the filled Jacobian's
 * transposed SpMV. nk_problem_destroy frees the problem, its modules and its pattern; nk_problem_jac_csr returns the pattern
 * the problem owns (do not destroy it); nk_problem_initial_guess gives zeros.
 * A source that does not compile is NK_E_INVALID with the contract and the compiler's log in nk_last_error.
 * Radius 2 (bit 16 of the stencil code): NK_GRID_STAR2, the 9 points (0,±1) (0,±2) (±1,0) (±2,0) and the centre with
 * dof = 1..2 (18 partials), and NK_GRID_DIAMOND2, the 13 points with |di| + |dj| <= 2 — the support of the discrete biharmonic
 * — with dof = 1. With them u(di, dj, c) takes di, dj ∈ {−2, …, 2}; a read outside the stencil's shape (STAR2: more than one
 * non-zero offset; DIAMOND2: |di| + |dj| > 2) returns NaN. A Dirichlet neighbour up to two layers outside the grid reads 0 and
 * has no column; a periodic index wraps by ± n; nx, ny >= 5, with both boundaries, so that the five offsets of a direction are
 * five distinct columns on the torus. Points in pattern order (ascending node index inside the grid), as (di, dj):
 *   STAR2     (0,−2) (0,−1) (−2,0) (−1,0) C (1,0) (2,0) (0,1) (0,2)
 *   DIAMOND2  (0,−2) (−1,−1) (0,−1) (1,−1) (−2,0) (−1,0) C (1,0) (2,0) (−1,1) (0,1) (1,1) (0,2)
 * Every program is compiled from one text, which starts with its stencil's point count and offsets, and with one full set of
 * options (-DNK_DIM, -DNK_NFIELDS, -DNK_DOF, -DNK_XLO … -DNK_ZHI, -DNK_CH, -DNK_GRID_SET, -DNK_GRID_DIRECT). Every other code
 * (2, 18, …) is NK_E_INVALID. */
enum { NK_GRID_STAR = 0, NK_GRID_BOX = 1, NK_GRID_STAR2 = 16, NK_GRID_DIAMOND2 = 17 }; /* stencil  */
/* The boundary is one int wherever it appears. 0 and 1 are the two uniform boundaries. NK_GRID_SIDES(xlo, xhi, ylo, yhi, zlo,
 * zhi) gives every side of every axis a kind of its own (4 bits each under the marker bit NK_GRID_SIDES_BIT); the z kinds are
 * for 3-D grids — leave them 0 in 2-D, a set one is NK_E_INVALID there, so a typo shows. A ghost node at distance k = 1..radius
 * outside a side of an axis of n nodes:
 *   NK_GRID_DIRICHLET0   reads 0 and has no column;
 *   NK_GRID_PERIODIC     wraps; both sides of the axis must be periodic, else NK_E_INVALID naming the axis;
 *   NK_GRID_MIRROR_NODE  the wall is the outermost node: −k -> k and n−1+k -> n−1−k (NumPy's `reflect`);
 *   NK_GRID_MIRROR_FACE  the wall is half a cell outside: −k -> k−1 and n−1+k -> n−k (NumPy's `symmetric`) — the zero-flux wall
 *                        of a cell-centred grid.
 * Axes are independent. A point that leaves the grid through a Dirichlet-0 side of ANY axis reads 0 and has no column, whatever
 * the other axes do (its field read is the field at the node itself, the rule above). Otherwise every axis is wrapped or
 * mirrored on its own, and u, v and the fields are read at the resulting node. A mirrored ghost is another unknown: the
 * Jacobian is the true dF/du, the partials of all stencil points of a row that land on one node are added into one entry
 * (in ascending point order) and the pattern holds that column once, columns ascending as before — at a mirror-node wall −1
 * and +1 both land on node 1, at a mirror-face wall −1 lands on the centre, the box at a corner mirrored in two axes puts four
 * points on one node. The side minimum stays 2·radius + 1: with it one reflection always lands inside the grid. A packed code
 * whose sides are all Dirichlet-0 (all periodic) IS code 0 (1): same pattern, same program options, same code objects. */
enum { NK_GRID_DIRICHLET0 = 0, NK_GRID_PERIODIC = 1, NK_GRID_MIRROR_NODE = 2, NK_GRID_MIRROR_FACE = 3 }; /* boundary */
#define NK_GRID_SIDES_BIT (1 << 24)
#define NK_GRID_SIDES(xlo, xhi, ylo, yhi, zlo, zhi)                                                                        \
  (NK_GRID_SIDES_BIT | ((xlo) & 15) | (((xhi) & 15) << 4) | (((ylo) & 15) << 8) | (((yhi) & 15) << 12) | (((zlo) & 15) << 16) | \
   (((zhi) & 15) << 20))
/* The CSR pattern of the Jacobian (host only, no device needed): rowptr dof·nx·ny + 1 entries, colind *nnz entries, 0-based,
 * columns ascending within a row. Every (stencil point in the domain) × (component) entry is kept — structural even where a
 * derivative is zero. colind = NULL (and / or rowptr = NULL) asks for the sizes only. */
int nk_grid_pattern(int64_t nx, int64_t ny, int dof, int stencil, int boundary, int32_t *rowptr, int32_t *colind, int64_t *nnz);
/* compile only (no device needed); *code_bytes = size of the two code objects together */
int nk_grid_compile_check(const char *source, int dof, int stencil, int boundary, int nparams, int64_t *code_bytes);
/* the code object of one of the two programs, for inspection (jac = 0: nk_grid_residual and nk_grid_jvp; 1: nk_grid_jac);
 * buf = NULL asks for the size only; no device needed */
int nk_grid_code_object(const char *source, int dof, int stencil, int boundary, int nparams, int jac, void *buf,
                        int64_t capacity, int64_t *bytes);
int nk_problem_create_grid(nk_ctx *ctx, const char *source, int64_t nx, int64_t ny, int dof, int stencil, int boundary,
                           const double *params, int nparams, nk_problem **out);

/* Three dimensions. The same three kernels, generated from a source written against the 3-D neighbourhood:
 *     template <typename T> __device__ void nk_point(const nk_nbhd3<T> &u, const nk_real *p, nk_site3 s, T *f);
 * with  u(di, dj, dk, c = 0)  component c at node (i + di, j + dj, k + dk), every offset ∈ {−1, 0, 1} (constants, or the
 *                             counters of `#pragma unroll` loops). An offset that is no point of the stencil returns NaN, as
 *                             in 2-D: with NK_GRID_STAR a read with more than one non-zero offset (an edge or a corner);
 *       s                     nk_site3 {i, j, k, nx, ny, nz};
 *       p, f, nk_real         as in 2-D.
 * Geometry: nx × ny × nz nodes, nx, ny, nz >= 3; unknown c of node (i, j, k) is element c·nx·ny·nz + (k·ny + j)·nx + i
 * (component-major, as in 2-D). NK_GRID_STAR is the 7-point star with dof = 1..4, NK_GRID_BOX the 27-point box with dof = 1:
 * a row has at most 28 partials (this cap replaces 2-D's 20 for these entry points only; no permitted combination spills —
 * the generated kernels have no private segment). The boundary — NK_GRID_DIRICHLET0 or NK_GRID_PERIODIC — applies to all three
 * directions; NK_GRID_SIDES gives each of the six sides its own kind. The pattern's 32-bit indices are checked: nx·ny·nz·dof·npts·dof <= INT32_MAX.
 * Stencil points are numbered by ascending node index inside the grid — star: (0,0,−1) (0,−1,0) (−1,0,0) C (1,0,0) (0,1,0)
 * (0,0,1); box: dk outermost, di innermost — and the pattern keeps every (point in the domain) × (component) entry in ascending
 * column order, as in 2-D. The object is the same NK_PROBLEM_USER problem owning its pattern: nk_problem_set_params,
 * nk_problem_jac_csr, nk_problem_initial_guess and nk_problem_destroy work unchanged. Float64. The kernels are
 * nk_grid3_residual, nk_grid3_jvp (jac = 0) and nk_grid3_jac (jac = 1); NK_GRID_FILL_DIRECT keeps its meaning.
 * Radius 2: NK_GRID_STAR2 is the 13-point star with dof = 1..2 (26 partials) — one offset ∈ {−2, …, 2}, the others 0, anything
 * else reads NaN — in the order (0,0,−2) (0,0,−1) (0,−2,0) (0,−1,0) (−2,0,0) (−1,0,0) C (1,0,0) (2,0,0) (0,1,0) (0,2,0) (0,0,1)
 * (0,0,2); nx, ny, nz >= 5. NK_GRID_DIAMOND2 (25 points in 3-D) is not offered: NK_E_INVALID. */
int nk_grid3_pattern(int64_t nx, int64_t ny, int64_t nz, int dof, int stencil, int boundary, int32_t *rowptr, int32_t *colind,
                     int64_t *nnz);
int nk_grid3_compile_check(const char *source, int dof, int stencil, int boundary, int nparams, int64_t *code_bytes);
int nk_grid3_code_object(const char *source, int dof, int stencil, int boundary, int nparams, int jac, void *buf,
                         int64_t capacity, int64_t *bytes);
int nk_problem_create_grid3(nk_ctx *ctx, const char *source, int64_t nx, int64_t ny, int64_t nz, int dof, int stencil,
                            int boundary, const double *params, int nparams, nk_problem **out);

/* Fields: read-only data on the grid. A problem created with nfields = 1..4 owns that many arrays of one double per node — a
 * previous time level for implicit time stepping, a variable coefficient, a source term, a mask — and compiles a source written
 * against one more argument:
 *     2-D: template <typename T> __device__ void nk_point(const nk_nbhd<T> &u, const nk_flds &a, const nk_real *p, nk_site s, T *f);
 *     3-D: template <typename T> __device__ void nk_point(const nk_nbhd3<T> &u, const nk_flds3 &a, const nk_real *p, nk_site3 s, T *f);
 * with  a(di, dj, k = 0)  (3-D: a(di, dj, dk, k = 0)) field k at the neighbouring node, as an nk_real. It is never a dual: fields
 *                         are constants of the differentiation, they add no column to the pattern and no partial to J·v.
 * Offsets and shape rule are the stencil's own: a read outside the shape (a corner of the star, |di| + |dj| > 2 of the diamond)
 * returns NaN, exactly as u does. Boundary rule for fields: at a periodic boundary the index wraps, as for u; outside a
 * Dirichlet boundary a field reads as THE FIELD AT THE NODE ITSELF (not 0: the clamped address the u load already computes,
 * without the select that zeroes u), so a face coefficient 0.5·(a(0,0) + a(1,0)) degenerates to a(0,0) at the wall; at a mirror
 * side a field is read at the mirrored node, as u is. A source that wants something else tests s.
 * Storage: field k of node m (m = j·nx + i, 3-D (k·ny + j)·nx + i) is element k·nn + m of one device buffer of nfields·nn
 * doubles which the problem owns; it is zero-filled at creation, so nothing is ever read uninitialised. nk_problem_set_field
 * copies nn doubles from host or device memory into field k on the context's stream and, like nk_problem_set_params, marks the
 * problem changed: a Jacobian cached for the same u belongs to the old field and is filled again. nk_problem_get_field copies
 * field k out. Both are NK_E_INVALID — the message names the value — for k outside 0..nfields−1, for a problem that is not a
 * compiled grid problem and for one created without fields; nfields outside 0..4 is NK_E_INVALID at creation.
 * nz = 0 makes the 2-D problem, nz >= 3 the 3-D one; nfields = 0 gives the program and the problem of nk_problem_create_grid /
 * nk_problem_create_grid3. Everything else is unchanged: stencils, dof limits, side minimums, p, the pattern (nk_grid_pattern /
 * nk_grid3_pattern: fields add no columns), Float64, kind NK_PROBLEM_USER, every consumer. -DNK_NFIELDS=<nfields> is
 * what tells the programs with fields from those without; the kernels keep their names and their thread map (one node per thread, 256
 * per workgroup), and the staged fill's LDS is unchanged. The field neighbourhood is loaded with u's, unconditionally; a load
 * whose value the source does not read is removed by the compiler, so declaring a field costs nothing until it is read.
 * Algorithmic bytes per unknown, r = number of distinct fields the source reads: residual 16 + 8·r/dof, J·v 24 + 8·r/dof, the
 * fill its figure + 8·r/dof. A source with the other contract is NK_E_INVALID with the contract that applies in the message. */
int nk_problem_create_grid_fields(nk_ctx *ctx, const char *source, int64_t nx, int64_t ny, int64_t nz, int dof, int stencil,
                                  int boundary, const double *params, int nparams, int nfields, nk_problem **out);
int nk_problem_set_field(nk_problem *P, int k, const double *data, int memspace);
int nk_problem_get_field(nk_problem *P, int k, double *out, int memspace);
/* compile only / the code object of one program, as nk_grid_compile_check and nk_grid_code_object; dim = 2 or 3; no device needed */
int nk_grid_fields_compile_check(const char *source, int dim, int dof, int stencil, int boundary, int nparams, int nfields,
                                 int64_t *code_bytes);
int nk_grid_fields_code_object(const char *source, int dim, int dof, int stencil, int boundary, int nparams, int nfields, int jac,
                               void *buf, int64_t capacity, int64_t *bytes);

/* Several ranks. nk_problem_create_grid, _grid3 and _grid_fields accept a context of R > 1 ranks (the call is then collective):
 * the grid is split into slabs along its OUTERMOST axis — y in 2-D, z in 3-D. Rank r owns the lines (3-D: planes)
 * [l0, l1) = nk_partition_range(n_outer, 1, R, r), the rule of the built-in grid problems; nl = l1 − l0, nn_loc = the slab's nodes.
 *   Local numbering   component-major on the slab: unknown c of slab node m is local element c·nn_loc + m, with
 *                     m = jl·nx + i in 2-D and m = (kl·ny + j)·nx + i in 3-D (jl, kl: the line, the plane within the slab).
 *   Global numbering  row_begin + local, row_begin = dof · (nodes of all lower slabs): one contiguous row range per rank (what
 *                     nk_csr_create_local needs, the convention of the multi-rank Brusselator), a permutation of the one-rank
 *                     numbering c·nn + node. Within a row of the pattern the columns ascend in this numbering: (owner rank,
 *                     component, node within the owner's slab).
 *   The site          handed to the source stays global: s.j (3-D: s.k) is the line's index on the whole grid and s.ny (s.nz)
 *                     the whole extent, so a source that computes coefficients from its position means what it meant.
 *   Refusal           every rank's slab holds at least radius + 1 lines — ghost lines then come from the adjacent ranks only and
 *                     a mirror at a physical side of the split axis lands inside the rank's own slab — else NK_E_INVALID naming
 *                     n_outer, R, the thinnest slab and the radius. R = 1 is exactly the problem of one rank.
 * Each rank compiles programs whose two sides of the split axis are its own: a physical Dirichlet or mirror side keeps its kind,
 * a cut between two ranks (both sides, if the axis is periodic) is a kind internal to the programs. A stencil point that leaves
 * the slab through a cut is in the domain and reads u, v and the fields from that side's ghost lines — `radius` lines per
 * component, exchanged through the context's halo exchange before each launch: the residual and the fill exchange u, J·v
 * exchanges u and v; stats.halo_exchanges counts them and both transports carry them. Fields are split like u:
 * nk_problem_set_field takes and nk_problem_get_field returns the rank's nn_loc doubles, and nk_problem_set_field exchanges the
 * field's ghost lines once, there — on several ranks it is a collective call. Through a cut a field reads the neighbour's value;
 * outside a physical Dirichlet side it still reads as at the node itself. Jᵀv goes through the filled pattern as on one rank.
 * The first three calls below are host only (no device): the slab [line_begin, line_end) and its rows of the pattern with
 * int64 columns in the global numbering (size query with NULL arrays, like nk_grid_pattern; nz is not read for dim = 2; it also
 * reports the refusal), and the programs of rank `rank` of `nranks` — (nranks, rank) decide which sides are cuts and the order
 * of the ghost zones among a row's columns; nranks = 1 gives the programs of the calls above, byte for byte.
 * nk_problem_grid_slab: the lines of a compiled grid problem's own slab ([0, n_outer) on one rank). */
int nk_grid_slab_pattern(int dim, int64_t nx, int64_t ny, int64_t nz, int dof, int stencil, int boundary, int nranks, int rank,
                         int64_t *line_begin, int64_t *line_end, int32_t *rowptr, int64_t *colind_global, int64_t *nnz);
int nk_grid_slab_compile_check(const char *source, int dim, int dof, int stencil, int boundary, int nparams, int nfields,
                               int nranks, int rank, int64_t *code_bytes);
int nk_grid_slab_code_object(const char *source, int dim, int dof, int stencil, int boundary, int nparams, int nfields, int nranks,
                             int rank, int jac, void *buf, int64_t capacity, int64_t *bytes);
int nk_problem_grid_slab(nk_problem *P, int64_t *line_begin, int64_t *line_end);

/* ---------------------------------------------------------------- compiled graph problems (kernel generation, full size)
 * A residual given node by node over ANY sparse adjacency — a network, an unstructured mesh — what the reference's user writes
 * as `f` with NonlinearFunction(f; jac_prototype = any sparse pattern). The user supplies a CSR graph of the nodes and HIP C++
 * source defining, per node, a function that loops over the node's edges:
 *
 *     template <typename T> __device__ void nk_node(const nk_nbrs<T> &u, const nk_real *p, nk_vertex s, T *f);
 *
 *       u.self(c = 0)      the node's own unknown c                u.deg()         its number of edges
 *       u.nbr(e, c = 0)    unknown c of the e-th neighbour, e a run-time loop counter in 0 .. deg() − 1
 *       u.node(e)          that neighbour's index                  u.w(e, k = 0)   datum k of that edge
 *       u.a(k = 0)         the node's own datum k                  u.an(e, k = 0)  the neighbour's node datum k
 *       s                  {i, nn, deg}: the node, the node count, the degree
 *       p                  the parameters;  f: the node's dof residuals (entries not written are zero);  nk_real is double
 *
 * Data are nk_real, never duals: constants of the differentiation. A k outside the declared count reads NaN — the project's
 * rule for a wrong source — and so do an e outside 0 .. deg() − 1 and a c outside 0 .. dof − 1 (node(e): −1). The source is
 * compiled by hiprtc behind the dual-number prelude with the grid programs' options (-O3 -ffp-contract=off -std=c++17, gfx950)
 * into nk_graph_residual and nk_graph_jvp (one node per thread; the JVP is exact: value from u, partial from v) and
 * nk_graph_jac (the fill, one slot per thread, below). A source that does not compile is NK_E_INVALID with this contract and
 * the compiler's log in nk_last_error.
 *
 * The graph: nn >= 1 nodes; rowptr[nn + 1] and colind[ne] host arrays, 0-based; columns strictly ascending within a row; no
 * self-loops (the node itself is always an argument of its residual and always a column); it may be structurally nonsymmetric
 * (a directed network) and ne may be 0. Anything else — a decreasing rowptr, a column outside 0 .. nn − 1, a duplicate or
 * descending column, a self-loop — is NK_E_INVALID, decided on the host before anything is compiled or allocated, with a
 * message that names the first offending row and the rule it breaks. Limits: dof = 1..4, nparams = 0..32, nedge and nnode =
 * 0..4 data arrays per edge and per node, dof·dof·(ne + nn) <= INT32_MAX. A context of more than one rank gets
 * NK_E_UNSUPPORTED: partitioning an arbitrary graph is not built.
 *
 * Numbering is component-major as everywhere: unknown c of node i is element c·nn + i. Edge datum k of edge e (its position
 * in colind) is element k·ne + e and node datum k of node i element k·nn + i of two device buffers the problem owns, both zero
 * at creation. nk_problem_set_graph_data (on_edges = 1: an edge datum of ne doubles, 0: a node datum of nn doubles) copies from
 * host or device on the context's stream and, like nk_problem_set_field, marks the problem changed, so a Jacobian cached for
 * the same u is filled again; nk_problem_get_graph_data copies out. A k out of range, or a problem that is not a compiled graph
 * problem, is NK_E_INVALID naming the value.
 *
 * The pattern: row (c, i) holds, for every component c2 in order, the node itself and its neighbours in ascending node order —
 * dof·(deg_i + 1) entries with ascending columns c2·nn + node, structural even where a derivative vanishes. The deg_i + 1
 * column nodes of node i are its slots; the self slot sits at spos_i = the number of neighbours smaller than i, edge e at
 * e + (e >= spos_i). All ne + nn slots are numbered node after node: slot s of node i is global slot rowptr[i] + i + s, and the
 * value of dF_c(i)/du_c2(slot s) is element c·dof·(ne + nn) + dof·(rowptr[i] + i) + c2·(deg_i + 1) + s. nk_graph_pattern
 * returns exactly this CSR (host only; NULL arrays: the sizes only), nk_problem_jac_csr the one the problem owns.
 *
 * Cost. Algorithmic bytes per node of the residual: 16·dof + 4 + deg·(4 + 8·r_e) + 8·r_n with r_e, r_n the data arrays the
 * source reads; the JVP adds 8·dof. nbr(e, c) is one gathered load u[c·nn + colind[e]]: neighbour values are expected from
 * cache, which holds for a bandwidth-reducing ordering of the nodes and not for a random one — the library does not reorder the
 * user's graph. The fill evaluates nk_node once per slot with unit seeds on the dof unknowns of that slot: Σ (deg_i + 1)·deg_i
 * edge terms, the price of a run-time degree with a compile-time dual width. No atomics; every sum runs in the source's own
 * edge order, so all three kernels are bit-reproducible. NK_GRAPH_FILL_NODE=1 in the environment at creation selects the A/B
 * form of the fill (one node per thread, the slots in an inner loop; slower, tools/graph_problem_bench.py).
 *
 * The object is an NK_PROBLEM_USER problem like a compiled grid problem: matrix-free GMRES, the concrete-J path, the coloured
 * assembly, Jᵀv through the transposed SpMV and every `precs` object take it; nk_problem_set_params replaces p,
 * nk_problem_initial_guess gives zeros, nk_problem_destroy frees everything. nk_gmres_set_multigrid_preconditioner refuses it
 * (NK_E_INVALID; the aggregation AMG object is the multigrid of a general CSR). */
int nk_graph_pattern(int64_t nn, const int32_t *rowptr, const int32_t *colind, int dof, int32_t *jrowptr, int32_t *jcolind,
                     int64_t *nnz);
int nk_graph_compile_check(const char *source, int dof, int nparams, int nedge, int nnode, int64_t *code_bytes);
/* the code object of one of the two programs, for inspection (jac = 0: nk_graph_residual and nk_graph_jvp; 1: nk_graph_jac);
 * buf NULL: the size only. Host only */
int nk_graph_code_object(const char *source, int dof, int nparams, int nedge, int nnode, int jac, void *buf, int64_t capacity,
                         int64_t *bytes);
int nk_problem_create_graph(nk_ctx *ctx, const char *source, int64_t nn, const int32_t *rowptr, const int32_t *colind, int dof,
                            const double *params, int nparams, int nedge, int nnode, nk_problem **out);
int nk_problem_set_graph_data(nk_problem *P, int on_edges, int k, const double *data, int memspace);
int nk_problem_get_graph_data(nk_problem *P, int on_edges, int k, double *out, int memspace);

/* ---------------------------------------------------------------- compiled element problems (kernel generation, full size)
 * A finite-element or finite-volume residual given ELEMENT BY ELEMENT on any mesh — in the reference the ordinary assembly loop
 * inside `f` with jac_prototype = the mesh's sparsity. An element (a triangle, a quad, a tet, a hex, a bar of a truss) reads the
 * unknowns and the data of its few nodes, does its quadrature once and contributes to the residuals of all its nodes. The user
 * supplies the connectivity and HIP C++ source defining, per element,
 *
 *     template <typename T> __device__ void nk_element(const nk_elemv<T> &u, const nk_real *p, nk_cell s, T *f);
 *
 *       u.at(a, c = 0)     unknown c at the element's a-th node, a = 0 .. NK_NPE − 1
 *       u.node(a)          that node's index
 *       u.x(a, k = 0)      node datum k at that node (coordinates, a source term, a nodal coefficient)
 *       u.w(k = 0)         datum k of the element (a conductivity, a thickness, a material number)
 *       s                  {e, ne, nn}: the element, the element count, the node count
 *       p                  the parameters;  nk_real is double
 *       f[a·NK_DOF + c]    the element's contribution to residual c of its a-th node; entries not written are zero
 *
 * NK_NPE and NK_DOF are visible to the source as macros. Data are nk_real, never duals: constants of the differentiation. An
 * a, c or k out of range reads NaN — the project's rule for a wrong source — and node(a) then gives −1. The source is compiled
 * by hiprtc behind the dual-number prelude with the graph programs' options (-O3 -ffp-contract=off -std=c++17, gfx950) and the
 * same code-object cache (options + source) into nk_elem_residual and nk_elem_jvp (one element per thread; the JVP is exact:
 * value from u, partial from v) and nk_elem_jac (one (element, local node b) pair per thread, unit seeds on the dof unknowns of
 * local node b, so the dual width is dof whatever npe is). A source that does not compile is NK_E_INVALID with this contract
 * and the compiler's log in nk_last_error. Write loops over a with compile-time bounds (`#pragma unroll`, a < NK_NPE): an f[]
 * or a local array indexed by a run-time value may be placed in scratch memory, which costs bandwidth, not correctness.
 *
 * The mesh: conn[ne·npe], int32, row-major — the nodes of element e are conn[e·npe + a]; all elements have one npe; nn nodes
 * (several element types, boundary terms and point terms in one mesh: "Several element blocks" below).
 * Limits: ne >= 1, npe = 2..8, dof = 1..4, npe·dof <= 16, nnode and nelem = 0..4 data arrays per node and per element,
 * nparams = 0..32; ne·(npe·dof)² and the pattern's entry count both fit in int32. Refused on the host (NK_E_INVALID) before
 * anything is compiled or allocated, the first offending element named: a node index outside 0 .. nn − 1, a node twice in one
 * element, and the limits. A node that is in no element is allowed: its rows hold the diagonal only (structural, value 0 unless
 * the unknown is fixed) and its residual is 0 unless it is fixed. A context of more than one rank gets NK_E_UNSUPPORTED.
 *
 * The pattern: two nodes are adjacent when they share an element, and the Jacobian's CSR is nk_graph_pattern of that node
 * graph — the same slots, the same value layout. nk_elem_adjacency returns the node graph (ascending columns, no self-loops;
 * NULL arrays: the sizes only), nk_elem_pattern the CSR (NULL arrays: the sizes only); both host only.
 *
 * Numbering is component-major: unknown c of node i is element c·nn + i. Node datum k of node i is element k·nn + i and element
 * datum k of element e element k·ne + e of two device buffers the problem owns, zero at creation; nk_problem_set_elem_data
 * (on_elements = 1: ne doubles, 0: nn doubles) copies from host or device and marks the problem changed, so a Jacobian cached
 * for the same u is filled again; nk_problem_get_elem_data copies out.
 *
 * Fixed unknowns (Dirichlet rows): nk_problem_set_elem_fixed takes mask[dof·nn] (int32, component-major, 0 = free) and
 * values[dof·nn] (NULL: zeros); default nothing fixed. A fixed row r has F_r = u_r − g_r, its row of J is the unit row on the
 * row's structural entries (1 on the diagonal, 0 on the others) and (Jv)_r = v_r. Columns of fixed unknowns stay in the free
 * rows: the matrix is nonsymmetric. Setting it invalidates a cached Jacobian; nk_problem_get_elem_fixed copies both arrays out
 * (either may be NULL). nk_problem_initial_guess gives zeros with the fixed values written in.
 *
 * Kernels. Every callback is two launches on the stream it is given, both inside the context's per-kernel event timing: the
 * generated kernel computes every element once and writes its npe·dof numbers (the fill: its (npe·dof)² numbers) into a buffer
 * the problem owns as coalesced streams — number q of element e at q·ne + e; the device copy of conn is node-major for the same
 * reason — and k_elem_gather, an ordinary kernel of the library, writes one output per thread: the sum of the row's (the
 * entry's) list of buffer positions in ascending element order, or what a fixed row holds. The lists are built on the host at
 * creation, one int32 per (element, a) and one per (element, a, b). No atomics, a fixed order: every result is bit-reproducible
 * from run to run. A node in very many elements is walked by one thread: correct, not fast.
 *
 * The object is an NK_PROBLEM_USER problem like a compiled graph problem: matrix-free GMRES, the concrete-J path, the coloured
 * assembly, Jᵀv through the transposed SpMV and every `precs` object take it; nk_problem_set_params replaces p,
 * nk_problem_destroy frees everything; nk_gmres_set_multigrid_preconditioner refuses it (NK_E_INVALID; the aggregation AMG
 * object is the multigrid of a general CSR). */
int nk_elem_adjacency(int64_t nn, int64_t ne, int npe, const int32_t *conn, int32_t *rowptr, int32_t *colind, int64_t *nedges);
int nk_elem_pattern(int64_t nn, int64_t ne, int npe, const int32_t *conn, int dof, int32_t *jrowptr, int32_t *jcolind,
                    int64_t *nnz);
int nk_elem_compile_check(const char *source, int npe, int dof, int nparams, int nnode, int nelem, int64_t *code_bytes);
/* the code object of one of the two programs, for inspection (jac = 0: nk_elem_residual and nk_elem_jvp; 1: nk_elem_jac);
 * buf NULL: the size only. Host only */
int nk_elem_code_object(const char *source, int npe, int dof, int nparams, int nnode, int nelem, int jac, void *buf,
                        int64_t capacity, int64_t *bytes);
int nk_problem_create_elements(nk_ctx *ctx, const char *source, int64_t nn, int64_t ne, int npe, const int32_t *conn, int dof,
                               const double *params, int nparams, int nnode, int nelem, nk_problem **out);
int nk_problem_set_elem_data(nk_problem *P, int on_elements, int k, const double *data, int memspace);
int nk_problem_get_elem_data(nk_problem *P, int on_elements, int k, double *out, int memspace);
int nk_problem_set_elem_fixed(nk_problem *P, const int32_t *mask, const double *values, int memspace);
int nk_problem_get_elem_fixed(nk_problem *P, int32_t *mask, double *values, int memspace);

/* Several element blocks in one mesh. One element problem made of nblocks = 1..8 BLOCKS: every block has its own connectivity
 * conn[k] (ne[k]·npe[k], row-major), its own npe[k], its own source sources[k] (its own nk_element) and its own nelem[k] = 0..4
 * element data; all blocks share nn, dof, p, the node data, the fixed-unknown mask, the pattern and the output vectors. This is
 * how a boundary term (Neumann, Robin, radiation: bars on the boundary edges of a triangulation, faces of a tet mesh), a mixed
 * mesh (triangles beside quads, tets beside hexes), a truss on top of a continuum and point terms are written: in the
 * reference, several loops inside `f`. A row of F, a row of J·v and an entry of J are the sums of the contributions of all
 * blocks in one fixed order — block 0's elements ascending, then block 1's, and so on, starting from 0 — without atomics:
 * bit-reproducible.
 *
 * The source of block k sees the contract above with NK_NPE and NK_NELEM of its own block, s = {e, ne, nn} with e and ne
 * counting within the block, u.w(k) its block's own element data, and the macro NK_BLOCK = k (0 in a plain problem). A source
 * that does not compile names its block ("element block 2 residual source does not compile") in front of the contract and the
 * log.
 *
 * Limits: per block ne >= 1, npe = 1..8 and npe·dof <= 16; npe = 1 is a point element (a nodal spring, a point load, a lumped
 * term) and adds no node pairs. dof²·Σ npe_k²·ne_k and the pattern's entry count fit in int32. Every refusal comes on the host
 * before anything is compiled or allocated and names the block and the first offending element: "block 2, element 17: node 301
 * (local node 1) outside 0..299". A context of more than one rank gets NK_E_UNSUPPORTED.
 *
 * The pattern: two nodes are adjacent when they share an element of any block; the CSR is nk_graph_pattern of that union graph.
 * A pair that only a bar block creates is a structural entry like any other. nk_elem_blocks_adjacency and
 * nk_elem_blocks_pattern are nk_elem_adjacency and nk_elem_pattern of the union (NULL arrays: the sizes only; host only).
 *
 * One block with npe >= 2 is nk_problem_create_elements: the same programs, buffers and launches. On any element problem
 * nk_problem_set_elem_data / nk_problem_get_elem_data with on_elements = 1 mean block 0 (0: the node data);
 * nk_problem_set_elem_block_data / nk_problem_get_elem_block_data address datum k of block `block` (ne[block] doubles) and
 * work on a one-block problem with block = 0. nk_problem_elem_blocks returns the block count and, for the first `cap` blocks,
 * ne, npe and nelem (any array may be NULL).
 *
 * Kernels. With TB = Σ npe_k·ne_k and TM = Σ npe_k²·ne_k, base_k and mbase_k the same sums over the blocks before k: number
 * (a, c) of element e of block k lives at c·TB + base_k + a·ne_k + e of the element-vector buffer and dF_(a,c)/du_(b,c2) at
 * (c·dof + c2)·TM + mbase_k + (a·npe_k + b)·ne_k + e of the element-matrix buffer — the component offset does not depend on
 * the block, every store is still one coalesced stream per register. A callback is one generated launch per block (compiled
 * with -DNK_ELEM_BLOCKS=1: the block's base and the total stride as two further arguments), on the stream it is given and in
 * the callback's profile family, and then ONE k_elem_gather launch (family elem_gather) over lists that walk the blocks in
 * order. nk_elem_block_code_object is nk_elem_code_object for the block form of block `block` = 0..7 (npe = 1 allowed). */
int nk_elem_blocks_adjacency(int64_t nn, int nblocks, const int64_t *ne, const int *npe, const int32_t *const *conn,
                             int32_t *rowptr, int32_t *colind, int64_t *nedges);
int nk_elem_blocks_pattern(int64_t nn, int nblocks, const int64_t *ne, const int *npe, const int32_t *const *conn, int dof,
                           int32_t *jrowptr, int32_t *jcolind, int64_t *nnz);
int nk_elem_block_code_object(const char *source, int block, int npe, int dof, int nparams, int nnode, int nelem, int jac,
                              void *buf, int64_t capacity, int64_t *bytes);
int nk_problem_create_element_blocks(nk_ctx *ctx, int64_t nn, int dof, int nblocks, const char *const *sources, const int64_t *ne,
                                     const int *npe, const int32_t *const *conn, const int *nelem, const double *params,
                                     int nparams, int nnode, nk_problem **out);
int nk_problem_set_elem_block_data(nk_problem *P, int block, int k, const double *data, int memspace);
int nk_problem_get_elem_block_data(nk_problem *P, int block, int k, double *out, int memspace);
int nk_problem_elem_blocks(nk_problem *P, int *nblocks, int cap, int64_t *ne, int *npe, int *nelem);

/* ---------------------------------------------------------------- GMRES (seam 1) */
/* restart_m: the restart length m, 1 <= m <= 63 (the dot-product kernels take at most 64 columns at once); restart_m <= 0 means 30;
 * restart_m >= 64 is NK_E_INVALID with a message that names the limit, before anything is allocated or launched. */
int nk_gmres_create(nk_ctx *ctx, int64_t n_local, int restart_m, int ortho, nk_gmres **out);
int nk_gmres_destroy(nk_gmres *G);
int nk_gmres_set_operator_csr(nk_gmres *G, nk_csr *A);                    /* cache.A = SparseMatrix   */
int nk_gmres_set_operator_jvp(nk_gmres *G, nk_problem *P, const double *u, int memspace); /* Stateful… */
int nk_gmres_set_operator_fn(nk_gmres *G, nk_matvec_fn fn, void *user);
/* on != 0: the operator of the next solves is AᵀA for the CSR / problem operator that is set (normal form: the
 * transposed half is the distributed transposed SpMV or the problem's VJP); the caller passes b = Aᵀ f. */
int nk_gmres_set_normal_form(nk_gmres *G, int on);   /* AbstractSciMLOperator    */
/* NK_ORTHO_SSTEP: number of basis columns per block, 1..16; 0 = automatic (15 with the Newton basis, 6 with the monomial
 * one). The last block of a cycle is cut to fit the restart length. */
int nk_gmres_set_block_size(nk_gmres *G, int s);
/* NK_ORTHO_SSTEP: basis of a block (nk_ss_basis) */
int nk_gmres_set_sstep_basis(nk_gmres *G, int basis);
/* Real bounds lo < hi of the operator's spectrum (its real part) for operators the library cannot bound itself — callback
 * and matrix-free operators. They place the Newton-basis shifts of NK_ORTHO_SSTEP; approximate bounds are fine (the
 * shifts only condition the block, the Krylov space is the same). lo = hi = 0 forgets them. */
int nk_gmres_set_spectrum_interval(nk_gmres *G, double lo, double hi);
/* NK_ORTHO_SSTEP diagnostics: the block size in effect (automatic sizes narrow 15 → 8 → 4 after a block lost rank), whether
 * the last solve built Newton-basis blocks, and how many blocks have lost rank so far (each made its cycle run again —
 * narrower, or column by column). Any pointer may be NULL. */
int nk_gmres_get_sstep_state(nk_gmres *G, int *block_size, int *newton_basis, int *breakdowns);
/* NK_ORTHO_SSTEP diagnostics: the bounds lo < hi of the spectrum the last solve placed its Newton-basis shifts on (Gershgorin
 * discs of a CSR operator, closed-form or caller's bounds). An error if the last solve built no Newton-basis blocks. Read it
 * before the next solve is prepared. */
int nk_gmres_get_sstep_interval(nk_gmres *G, double *lo, double *hi);
/* Damped normal form: the operator becomes AᵀA + lambda·diag(d) (d: DEVICE vector of local length n, kept by reference;
 * NULL switches the damping off) — `dampen_jacobian!!(J_cache, JᵀJ, λ·DᵀD)` of DampedNewtonDescent's :normal_form mode
 * (lib/NonlinearSolveBase/src/descent/damped_newton.jl:297-313,356-370) without assembling JᵀJ. */
int nk_gmres_set_normal_form_damping(nk_gmres *G, const double *d_diag, double lambda);
/* Shifted operator: A + sigma·I for the operator that is set (0 switches it off) — `J + D` for a matrix-free Jacobian
 * operator under DampedNewtonDescent (`dampen_jacobian!!(::Any, J::AbstractSciMLOperator, D) = J + D`, damped_newton.jl:349). */
int nk_gmres_set_shift(nk_gmres *G, double sigma);
/* … and A + sigma·diag(m) with a DEVICE vector m of local length n (kept by reference; NULL = identity): the damping α⁻¹ M of
 * PseudoTransient(; mass_matrix = Diagonal(m)) (pseudo_transient.jl:102-120,149). */
int nk_gmres_set_shift_weights(nk_gmres *G, const double *d_m);
/* ---- preconditioners: the `precs(A, p) -> (Pl, Pr)` hook of the LinearSolve interface
 * (lib/NonlinearSolveBase/src/linear_solve.jl:195-199 wrap_preconditioners; test/Core/core_tests__item21.jl:10-18;
 *  docs/src/tutorials/large_systems.md:252-316, whose `precs` return `(Pl, I)`). GMRES solves Pl⁻¹ A Pr⁻¹ (Pr x) = Pl⁻¹ b:
 * the Arnoldi process runs on Pl⁻¹ A Pr⁻¹, and with a left preconditioner the stopping test
 * ‖Pl⁻¹(b − A x)‖ ≤ atol + rtol·‖Pl⁻¹(b − A x₀)‖ and nk_gmres_info.rnorm0 / rnorm refer to the PRECONDITIONED residual, as in
 * Krylov.jl's gmres [EXT]. Either side takes a callback (device or host pointers) or a built-in object; fn / P = NULL removes
 * that side. Callbacks must be linear maps y = P⁻¹ x. */
/* right preconditioner x = Pr⁻¹ z applied as a device callback */
int nk_gmres_set_right_preconditioner(nk_gmres *G, nk_matvec_fn fn, void *user);
/* left preconditioner y = Pl⁻¹ r applied as a device callback */
int nk_gmres_set_left_preconditioner(nk_gmres *G, nk_matvec_fn fn, void *user);
int nk_gmres_set_left_preconditioner_host(nk_gmres *G, nk_matvec_fn fn, void *user);
/* a built-in preconditioner object (below) on either side; the object stays the caller's (it must outlive its use here,
 * and nk_precond_update is the caller's to call when the matrix values change) */
typedef enum { NK_SIDE_RIGHT = 0, NK_SIDE_LEFT = 1 } nk_side;
typedef struct nk_precond nk_precond;
int nk_gmres_set_preconditioner(nk_gmres *G, int side, nk_precond *P);

/* Preconditioner objects built from a CSR matrix (csrc/nk_precond.hip) — what `precs(A, p)` returns for a general sparse
 * Jacobian (the reference's tutorial fills the slot with IncompleteLU.ilu(W) / an algebraic multigrid):
 *   Jacobi: M = diag(A).  ILU(0): A ≈ LU on the pattern of A, no fill, no pivoting, of the rank's LOCAL square block (halo
 *   columns dropped: block-Jacobi ILU(0) across ranks, no communication in the apply). Rows are scheduled by dependency levels;
 *   NK_ILU_NATURAL keeps the matrix's ordering (the classical preconditioner; a lexicographic stencil has 2n − 1 levels, walked
 *   inside one persistent workgroup — milliseconds per application at n = 1024²), NK_ILU_MULTICOLOR permutes the rows by a
 *   greedy colouring of the pattern (as many levels as colours, one wide launch each: the GPU form).
 * nk_precond_update refactorises for the matrix's current values; NK_E_SINGULAR on a zero pivot. x, y: local length n. */
typedef enum { NK_PRECOND_JACOBI = 1, NK_PRECOND_ILU0 = 2, NK_PRECOND_AMG = 3, NK_PRECOND_ILUT = 4 } nk_precond_kind;
typedef enum { NK_ILU_NATURAL = 0, NK_ILU_MULTICOLOR = 1 } nk_ilu_ordering;
int nk_precond_create_jacobi(nk_csr *A, nk_precond **out);
int nk_precond_create_ilu0(nk_csr *A, int ordering, nk_precond **out);
/* ILU with a drop tolerance — the tutorial's `incompletelu(W, p) = (ilu(W, τ = 50.0), I)` (docs/src/tutorials/large_systems.md:252-260;
 * IncompleteLU.jl [EXT]): Crout ILU (Li, Saad, Chow 2003), A ≈ (I + L) U with fill; an off-diagonal entry of U's row k / L's column
 * k is kept if its magnitude BEFORE the division by the pivot is ≥ tau (absolute; tau = 0: the complete LU without pivoting). The
 * factorisation runs on the HOST for every nk_precond_update (its pattern depends on the numbers — the reference's runs on the
 * CPU as well), of the rank's local block; the triangular solves of every application run on the device, level-scheduled from the
 * factors' pattern. nk_precond_ilu0_factors returns its factors as well. NK_E_SINGULAR on a zero pivot. */
int nk_precond_create_ilut(nk_csr *A, double tau, nk_precond **out);
/* Aggregation algebraic multigrid built from the matrix alone (csrc/nk_amg.hip) — the tutorial's
 * `precs = (A, p) -> (aspreconditioner(ruge_stuben(A)), I)` slot (docs/src/tutorials/large_systems.md:276-316): pairwise
 * aggregation (`passes` times per level: aggregates of ≤ 2^passes rows; strength threshold `theta`) fixed at creation from the
 * values of that moment, piecewise-constant transfers, Galerkin coarse matrices, `nu` Chebyshev steps on D⁻¹A over
 * [λmax / cheb_ratio, λmax] before and after, the coarse correction over-corrected by `overcorrection`, levels down to
 * ≤ coarse_max (≤ 128) rows, inverted densely. nk_precond_update keeps the aggregates and refreshes every number on the
 * device (Galerkin sums, D⁻¹, Gershgorin bounds, the coarse inverse) for the matrix's current values. A fixed linear
 * operator: usable as Pl or Pr. Several ranks: the rank's local block (block-Jacobi AMG). params NULL or zero fields:
 * defaults (nu 2, passes 2, theta 0.25, overcorrection 1.8, cheb_ratio 4, coarse_max 128, matching 0). Every other value is
 * taken as given or refused with NK_E_INVALID, never replaced: a negative (or NaN) field, cheb_ratio in (0, 1], nu > 16,
 * passes > 4, coarse_max > 128, matching outside 0..2 (0 automatic, 1 the host's sequential pass, 2 the device's handshaking).
 * A matrix without rows (a rank may own none) is accepted: one level of 0 rows with the bound 1.0, nothing is launched by
 * create, update or apply. Columns sorted and unique within every row (NK_E_INVALID otherwise); NK_E_SINGULAR on a zero,
 * missing or non-finite diagonal entry on any level and on a singular coarsest matrix — from nk_precond_update as well, after
 * which nk_precond_apply refuses until an update succeeds. */
typedef struct nk_amg_params {
  int32_t nu, passes, coarse_max, matching;
  double theta, overcorrection, cheb_ratio;
} nk_amg_params;
int nk_amg_params_default(nk_amg_params *p);
int nk_precond_create_amg(nk_csr *A, const nk_amg_params *params, nk_precond **out);
/* how the aggregates were formed: 1 = the sequential pairwise pass (host set-up), 2 = handshaking (device set-up) */
int nk_precond_amg_matching(nk_precond *P, int *matching);
/* the hierarchy, for inspection: *levels (coarsest included); sizes / nnzs / lmax: up to `cap` entries each (NULL: skipped) */
int nk_precond_amg_info(nk_precond *P, int *levels, int cap, int64_t *sizes, int64_t *nnzs, double *lmax);
/* row → coarse row of level `level` (`count` = that level's rows; the coarsest level has none: NK_E_INVALID) */
int nk_precond_amg_aggregates(nk_precond *P, int level, int32_t *agg, int64_t count);
/* level `level`'s matrix itself, for inspection (owned by the hierarchy: do not destroy; valid until the preconditioner goes;
 * its values are those of the last nk_precond_update). Level 0 is the caller's matrix, or on several ranks the private copy of
 * the rank's local square block. A level outside 0 .. levels − 1: NK_E_INVALID. */
int nk_precond_amg_level_matrix(nk_precond *P, int level, nk_csr **out);
int nk_precond_update(nk_precond *P);
int nk_precond_apply(nk_precond *P, const double *x, double *y, int memspace);   /* y = M⁻¹ x */
int nk_precond_info(nk_precond *P, int *kind, int *levels_lower, int *levels_upper, int *ncolors);
/* the ILU(0) factors in the (permuted) ordering, for inspection: CSR of the local block — L strictly below the diagonal
 * (unit diagonal implied), U on and above — and perm[permuted row] = original row. Any pointer may be NULL. */
int nk_precond_ilu0_factors(nk_precond *P, int64_t *nnz, int32_t *rowptr, int32_t *col, double *val, int32_t *perm);
int nk_precond_destroy(nk_precond *P);
/* The same two hooks for operators that live in HOST memory (a Julia `mul!` on plain Arrays): the callback receives host
 * pointers, the library stages the vectors through pinned buffers around every call (2 × 8 n bytes over PCIe each). */
int nk_gmres_set_operator_fn_host(nk_gmres *G, nk_matvec_fn fn, void *user);
int nk_gmres_set_right_preconditioner_host(nk_gmres *G, nk_matvec_fn fn, void *user);
/* Built-in right preconditioner M⁻¹ = p_d(A): `degree` steps of the Chebyshev iteration on [lambda_min, lambda_max]
 * (operator applications only: no inner products, no all-reduce). lambda_max = 0 ⇒ the dominant eigenvalue is
 * bounded by Gershgorin (concrete CSR) or estimated by 30 power iterations ×1.15 (matrix-free / callback
 * operators) and lambda_min = lambda_max / ratio. The interval must not contain 0
 * (negative-definite operators are fine). degree ≤ 0 removes it. Call after the operator is set. */
int nk_gmres_set_chebyshev_preconditioner(nk_gmres *G, int degree, double lambda_min, double lambda_max, double ratio);
int nk_gmres_get_chebyshev_interval(nk_gmres *G, double *lambda_min, double *lambda_max);
/* Built-in right preconditioner M⁻¹ = one geometric multigrid V-cycle on the Jacobian of a BRATU2D problem linearised at u
 * (level operators by rediscretisation, bilinear transfers between non-nested grids, `nu` Chebyshev smoothing steps before
 * and after, banded LU on the coarsest grid of side ≤ coarse_max; 0 → 2 and 31) — the device counterpart of an algebraic-
 * multigrid `precs` (docs/src/tutorials/large_systems.md:244-316). Mesh-independent Krylov iteration counts. Call it again
 * for every new linearisation point; nu ≤ 0 or P == NULL removes it. Single rank.
 *
 * A compiled grid problem (nk_problem_create_grid …, one rank; more ranks: NK_E_INVALID) gets the same V-cycle for its own PDE
 * (csrc/nk_gridmg.hip): 2-D and 3-D, every stencil, dof <= 4, fields, every combination of side kinds.
 *   levels     by rediscretisation: level l is the same problem — same source, options and p, the fine problem's code objects
 *              loaded again — on smaller sides; A_l is its Jacobian fill at u_l = R u_{l−1}, its fields are the restriction of
 *              the finer level's. Every call restricts u and the fields, copies the current p, refills every A_l and refactors
 *              the coarsest level, so nk_problem_set_field / nk_problem_set_params between solves are picked up.
 *   CONTRACT   a source used with the multigrid takes its spacing from s.nx, s.ny, s.nz (the level it runs on), not from p.
 *              A source that does not follow this gets a poor preconditioner, not a wrong answer; the AMG object remains for it.
 *   geometry   per axis (nk_grid_mg_axis), in units of the fine spacing: a side's offset a is 1 (Dirichlet-0: the wall is one
 *              spacing outside the outermost node), 0 (mirror_node) or 1/2 (mirror_face); L = n − 1 + a_lo + a_hi, node i sits at
 *              a_lo + i, nc = floor(L/2 + 1.5 − a_lo − a_hi); periodic: L = n, nc = floor(n/2 + 0.5). An axis is coarsened while
 *              n > coarse_max and nc >= the stencil's smallest side (3; radius 2: 5); the hierarchy ends when none is.
 *   transfers  tensor products of the 1-D tables: linear interpolation at the nodes' positions, restriction = its row-normalised
 *              transpose (residuals, u and fields alike), component by component.
 *   smoother   nu Chebyshev steps on D⁻¹A_l over [rho/4, rho], rho = max_i sum_j |a_ij| / |a_ii| (computed at every call); a zero
 *              or non-finite diagonal entry fails the call with the level and the row. Coarsest level: the banded LU.
 * coarse_max < 3 → 8 for a compiled grid problem. A solver object holds one hierarchy, that of its last call: a call with a
 * compiled grid problem builds it again when the problem, nu or coarse_max differ from the call that built it, and a call with a
 * problem of the other kind (built-in after compiled, or the reverse) replaces it. For BRATU2D and BRUSSELATOR2D the hierarchy is
 * built by the first call and later calls only re-linearise it: nu, coarse_max and P of those calls are not looked at again. */

int nk_gmres_set_multigrid_preconditioner(nk_gmres *G, nk_problem *P, const double *u, int memspace, int nu, int coarse_max);
/* The folded prolongation table of one axis of n nodes with the side kinds (lo_kind, hi_kind) onto its coarser axis of *nc
 * nodes (host only, like nk_grid_pattern): fine node i takes w[2i] of coarse node idx[2i] and w[2i + 1] of idx[2i + 1], where
 * t = (a_lo + i)·(nc − 1 + a_lo + a_hi)/L − a_lo (periodic: i·nc/n), J0 = floor(t), the weights 1 − (t − J0) on J0 and t − J0 on
 * J0 + 1, a weight within 1e-12 of 0 or 1 snapped to the node. A coarse index outside 0 … nc−1 goes through the grid's own side
 * map (Dirichlet-0 drops it, periodic wraps, the mirrors reflect); two weights landing on one coarse node are added into the
 * first entry. A dropped, merged or zero-weight entry has the index −1 and the weight 0. idx = w = NULL: only *nc. */
int nk_grid_mg_axis(int64_t n, int lo_kind, int hi_kind, int64_t *nc, int32_t *idx, double *w);
/* The hierarchy behind nk_gmres_set_multigrid_preconditioner on a compiled grid problem: *levels, and for the first `cap` of
 * them (arrays nullable) the sides nx, ny, nz (3 per level; 2-D: nz = 1), the unknowns, the non-zeros of A_l and rho.
 * nk_gmres_multigrid_level_matrix: A_l itself (owned by the hierarchy: do not destroy; valid until the solver object goes).
 * nk_gmres_multigrid_level_field: a copy of field k of level l (n/dof doubles). */
int nk_gmres_multigrid_levels(nk_gmres *G, int *levels, int cap, int64_t *sides, int64_t *n, int64_t *nnz, double *rho);
int nk_gmres_multigrid_level_matrix(nk_gmres *G, int level, nk_csr **out);
int nk_gmres_multigrid_level_field(nk_gmres *G, int level, int k, double *out, int memspace);
/* Solve A x = b. use_x0 = 0 ⇒ zero initial guess (our protocol); 1 ⇒ x holds x0.
 * Stop when ‖r‖₂ ≤ atol + rtol‖r0‖₂ or after maxiter Arnoldi steps; fixed_iters>0 overrides both.
 *  - use_x0 = 1 with a right preconditioner (callback, object, Chebyshev or multigrid) is NK_E_UNSUPPORTED ("not supported"):
 *    nothing is iterated, x keeps x0, and the object serves the next solve as before.
 *  - With a left preconditioner every norm of the solve is the preconditioned one: info.rnorm0 = ‖Pl⁻¹(b − A x0)‖,
 *    info.rnorm = the recurrence estimate of ‖Pl⁻¹(b − A x)‖, and atol / rtol are measured against those.
 *  - n_local = 0 on one rank: a converged empty solve — NK_OK, info = {0 iterations, 0 restarts, converged = 1, failed = 0,
 *    rnorm0 = rnorm = 0}; nothing is launched, no callback runs, b and x are not read and may be NULL. (On several ranks a rank
 *    without rows takes part in the collectives like every other.) */
int nk_gmres_solve(nk_gmres *G, const double *b, double *x, int memspace, int use_x0,
                   double atol, double rtol, int maxiter, int fixed_iters, nk_gmres_info *info);

/* ---------------------------------------------------------------- direct factorisation (seam 1, `linsolve = nothing`)
 * Direct factorisation of a concrete banded sparse J on the device; factor once, solve many
 * (reuse_A_if_factorization, lib/NonlinearSolveBase/ext/NonlinearSolveBaseLinearSolveExt.jl:81-86). Single rank.
 * Engine (nk_lu_engine): block cyclic reduction — batched dense blocks of order b = bandwidth rounded to 32 (b <= 512) on FP64
 * MFMA, log2(n/b) dependent levels — or, for matrices of fewer than four block rows, a right-looking band LU (kl <= 447,
 * ku <= 512; a matrix of fewer block rows with 447 < kl <= 512 goes to block cyclic reduction). Pivots: on the diagonal first; the cyclic-reduction engine switches to row pivoting inside its dense
 * blocks when a diagonal pivot vanishes (NK_BCR_PIVOT=auto|always|never); *ok = 0 when the factorisation still broke down. */
int nk_lu_create(nk_csr *A, nk_lu **out);
int nk_lu_destroy(nk_lu *F);
int nk_lu_factor(nk_lu *F, nk_csr *A, int *ok);
int nk_lu_solve(nk_lu *F, const double *b, double *x, int memspace);
int nk_lu_info(nk_lu *F, int *kl, int *ku, int64_t *band_bytes);   /* band_bytes: device memory held by the factorisation */
/* which engine the factorisation object runs on: 0 = right-looking band LU (a chain of n/32 dependent block columns),
 * 1 = block cyclic reduction (log2(n/b) levels of batched dense b x b algebra on FP64 MFMA; chosen automatically when the
 * matrix has >= 4 block rows of order b = bandwidth rounded to 32, b <= 512, or when kl > 447 and b <= 512 whatever the
 * number of block rows; NK_DIRECT=band in the environment forces 0 wherever the band LU can hold the matrix);
 * `block` = b (0 for the band LU), `levels` = number of reduction levels. */
int nk_lu_engine(nk_lu *F, int *engine, int *block, int *levels);

/* ---------------------------------------------------------------- Newton / TrustRegion (seam 3) */
int nk_options_default(nk_options *opts);
int nk_solver_init(nk_problem *P, const double *u0, int memspace, const nk_options *opts,
                   nk_solver **out);                       /* SciMLBase.__init */
int nk_solver_destroy(nk_solver *S);
int nk_solver_step(nk_solver *S);                          /* CommonSolve.step!  */
/* step!(cache; recompute_jacobian, evaluate_residual) (lib/NonlinearSolveBase/src/solve.jl:835-859 →
 * lib/NonlinearSolveFirstOrder/src/solve.jl:325-465). recompute_jacobian: -1 = nothing (the algorithm decides), 0, 1.
 * evaluate_residual = 0 is a HINT: honoured only when nk_solver_supports_deferred_residual says 1 (unglobalised Newton
 * step, AbsTerminationMode / AbsNormTerminationMode, no trace — FirstOrder/src/solve.jl:303-316); the step then ends
 * right after u += δu and nk_solver_refresh_residual (= refresh_residual!, :318-324) evaluates f(u) and runs the
 * termination check on demand. step and solve settle an outstanding deferral themselves. */
int nk_solver_step_ex(nk_solver *S, int recompute_jacobian, int evaluate_residual);
int nk_solver_supports_deferred_residual(nk_solver *S, int *yes);
int nk_solver_refresh_residual(nk_solver *S);
int nk_solver_solve(nk_solver *S, int *retcode);           /* CommonSolve.solve! */
int nk_solver_reinit(nk_solver *S, const double *u0, int memspace,
                     const double *params, int nparams);   /* SciMLBase.reinit!(cache, u0; p) */
/* PseudoTransient(; mass_matrix = Diagonal(m)) (pseudo_transient.jl:37-57): damping α⁻¹·diag(m); m has the local length of u,
 * is copied, and must be set before the first step (the reference fixes it at init). NULL returns to the identity. */
int nk_solver_set_mass_matrix_diagonal(nk_solver *S, const double *m, int memspace);
int nk_solver_get_u(nk_solver *S, double *u, int memspace);
int nk_solver_get_resid(nk_solver *S, double *f, int memspace);
int nk_solver_get_stats(nk_solver *S, nk_stats *stats);
/* The `precs(A, p) -> (Pl, Pr)` hook at solver level (KrylovJL_GMRES(precs = …); test/Core/core_tests__item21.jl:10-37):
 * `fn` is called once when it is installed — LinearSolve evaluates precs when the linear cache is built [EXT] — and then
 * right after every Jacobian refresh (a new `A` marks the LinearSolve cache fresh: lib/NonlinearSolveBase/ext/
 * NonlinearSolveBaseLinearSolveExt.jl:64-111), before that step's linear solve; never by nk_solver_reinit. It receives the
 * solver's GMRES object — install Pl / Pr on it with nk_gmres_set_left/right_preconditioner(_host) or
 * nk_gmres_set_preconditioner —, the concrete Jacobian (NULL on the matrix-free path) and the iterate (DEVICE pointer, local
 * length n: the `u` of LinearSolveParameters(u, p)). Non-zero return = NK_E_CALLBACK. fn = NULL removes the hook. */
typedef int (*nk_precs_fn)(void *user, nk_gmres *G, nk_csr *A, const double *u);
int nk_solver_set_precs(nk_solver *S, nk_precs_fn fn, void *user);
/* the solver's GMRES object and concrete Jacobian (NULL where the linsolve has none), e.g. to build preconditioner objects on */
nk_gmres *nk_solver_gmres(nk_solver *S);
nk_csr *nk_solver_jacobian(nk_solver *S);
int nk_solver_get_retcode(nk_solver *S, int *retcode, int *nsteps, int *force_stop);
/* NK_ALG_LIMITED_MEMORY_BROYDEN: the state of the low-rank inverse Jacobian (nk_stats has no slot for it): resets counted so
 * far, updates since the last reset (`idx`; min(idx, threshold) columns are in use), the scaling a of a·I + U Vᵀ, the
 * threshold in effect, and the reset test's two counters. Any pointer may be NULL. NK_E_INVALID for another algorithm. */
int nk_solver_get_lbroyden_state(nk_solver *S, int *nresets, int *idx, double *a, int *threshold, int *since_du,
                                 int *since_dfu);
/* NK_ALG_BROYDEN, NK_ALG_KLEMENT: resets counted so far, the scaling the last (re)initialisation used (Broyden: a = 1/α of
 * J⁻¹ = a·I; Klement: α of J = α·1), the reset test's two counters (0 for Klement) and the steps since the last reset. Any
 * pointer may be NULL. NK_E_INVALID for another algorithm. */
int nk_solver_get_qn_state(nk_solver *S, int *nresets, double *a, int *since_du, int *since_dfu, int *steps_since_reset);
/* NK_ALG_BROYDEN: the inverse Jacobian as it stands, row-major n×n with leading dimension ldo >= n (it exists from the first step
 * on: NK_E_INVALID before), or its n diagonal entries for the diagonal structure; NK_ALG_KLEMENT: the n diagonal entries of J. */
int nk_solver_get_broyden_inverse(nk_solver *S, double *out, int64_t ldo, int memspace);
/* NK_ALG_DFSANE: the spectral coefficient σ the next step starts from, the step length of the last step with its sign (+α₊ or
 * −α₋; 0 before the first step, NaN after a failed search), the residual evaluations of the last line search and of all of
 * them, the history length M and the merit history itself (`history`: room for 32 doubles, M are written). Any pointer may
 * be NULL. NK_E_INVALID for another algorithm. */
int nk_solver_get_dfsane_state(nk_solver *S, double *sigma, double *alpha, int *trials, int *total_trials, int *M,
                               double *history);
int nk_solver_get_scalars(nk_solver *S, double *fnorm_inf, double *trust_region, double *eta);
int nk_solver_get_trace(nk_solver *S, nk_trace_entry *rows, int capacity, int *nrows);
/* one call: init + solve + results (what SciMLBase.__solve of the extension algorithm does) */
int nk_newton_solve(nk_problem *P, const double *u0, int memspace, const nk_options *opts,
                    double *u_out, double *resid_out, nk_stats *stats, int *retcode);

/* ---------------------------------------------------------------- ensembles of small systems (kernel generation)
 * The reference's "GPU acceleration over large parameter searches" (docs/src/tutorials/nonlinear_solve_gpus.md:70-176):
 * SimpleNewtonRaphson (lib/SimpleNonlinearSolve/src/raphson.jl:39-83) for thousands of small (n ≤ 64) systems
 * f(u, p_b) = 0, one system per GPU thread. `source` is HIP C++ defining
 *     template <typename T> __device__ void nk_f(const T *u, const double *p, T *f);
 * (and, with flags & NK_BATCH_ANALYTIC_JAC, `__device__ void nk_jac(const double *u, const double *p, double *J)`, row-major
 * n×n). It is compiled at run time (hiprtc, gfx950) with the solver kernel; without nk_jac the Jacobian comes from forward-mode
 * dual numbers (AutoForwardDiff, the reference default). Semantics per system: iszero(f(u0)) ⇒ Success; δ = J \ f (partial
 * pivoting), u −= δ, then AbsNormTerminationMode(maximum∘abs) on the residual of the previous iterate; default abstol
 * eps^(4/5), maxiters 1000; per-system retcode (NK_RET_SUCCESS | NK_RET_MAXITERS) and iteration count.
 * Float32 (flags & NK_BATCH_FLOAT32, the tutorial's element type): every kernel runs in single precision, constants and the
 * default abstol eps(Float32)^(4/5) = 2.8909994e-6 included. The source then writes `nk_real` (= float) where it wrote double:
 *     template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f);
 *     __device__ void nk_jac(const nk_real *u, const nk_real *p, nk_real *J);
 * (a source written with nk_real compiles in both modes; one written with `const double *p` fails in Float32 mode with the
 * contract in nk_last_error). Such an object is solved through the _f32 entry points, which take float arrays; scalar
 * arguments stay double and are rounded to float (T(abstol)). Calling an object through the other precision's entry point is
 * NK_E_INVALID. nk_batch_compile_check compiles only (no device needed).
 * Medium systems, 8 < n <= 64, run one system per WAVEFRONT where such a kernel exists (nk_batch_newton_wave,
 * nk_batch_trust_region_wave: lane j owns column j of the dual-number Jacobian; nk_jac is not used by them). flags &
 * NK_BATCH_PER_THREAD switches that off for an object: no wavefront module is built or used and every method runs one system
 * per thread (the A/B handle; nk_batch_last_kernel tells which kernel ran). */
enum { NK_BATCH_ANALYTIC_JAC = 1, NK_BATCH_FLOAT32 = 2, NK_BATCH_PER_THREAD = 4 };   /* bits of `flags` */
int nk_batch_compile_check(const char *source, int n, int nparams, int flags, int64_t *code_bytes);
/* the compiled code object of one kernel set (wave = 0: nk_batch_newton and nk_batch_trust_region; 1: the one-system-per-
 * wavefront nk_batch_newton_wave; 2: the one-system-per-wavefront nk_batch_trust_region_wave; wave > 2 is NK_E_INVALID), for
 * inspection; *bytes gets its size, buf = NULL asks for the size only */
int nk_batch_code_object(const char *source, int n, int nparams, int flags, int wave, void *buf, int64_t capacity,
                         int64_t *bytes);
int nk_batch_create(nk_ctx *ctx, const char *source, int n, int nparams, int flags, nk_batch **out);
int nk_batch_destroy(nk_batch *B);
/* the name of the kernel the last solve on B launched ("nk_batch_newton_wave", "nk_batch_trust_region", ...): "" before any
 * solve, NULL for a NULL object. The string is static. */
const char *nk_batch_last_kernel(nk_batch *B);
/* u0: n doubles shared by all systems (u0_per_system = 0) or nbatch×n; p: nbatch×nparams; outputs nbatch×n, nbatch×n,
 * nbatch, nbatch (retcode/iters nullable); abstol ≤ 0 and maxiters ≤ 0 select the defaults. */
int nk_batch_solve(nk_batch *B, int64_t nbatch, const double *u0, int u0_per_system, const double *p, int memspace,
                   double abstol, int maxiters, double *u_out, double *resid_out, int32_t *retcode_out, int32_t *iters_out);
int nk_batch_solve_f32(nk_batch *B, int64_t nbatch, const float *u0, int u0_per_system, const float *p, int memspace,
                       double abstol, int maxiters, float *u_out, float *resid_out, int32_t *retcode_out, int32_t *iters_out);
/* SimpleTrustRegion (lib/SimpleNonlinearSolve/src/trust_region.jl:57-229, default radius update) per system; thresholds and
 * factors ≤ 0, max_shrink_times < 0 select the reference defaults (1e-4, 0.25, 0.75, 0.25, 2, 32). Retcodes: NK_RET_SUCCESS,
 * NK_RET_MAXITERS, NK_RET_SHRINK_THRESHOLD_EXCEEDED.
 * For 8 < n <= 64 (from NK_BATCH_TR_WAVE_MIN_N of nk_batch.hip on) the first such solve on an object compiles and loads
 * nk_batch_trust_region_wave, a module of its own, and this and later solves launch it; with NK_BATCH_PER_THREAD, at other
 * n, or if that module does not build, nk_batch_trust_region runs, one system per thread. The two differ at rounding level
 * only: column instead of row pivoting in the LU, ‖Jδ‖² for δᵀJᵀJδ, and butterfly instead of sequential sums. */
int nk_batch_solve_trust_region(nk_batch *B, int64_t nbatch, const double *u0, int u0_per_system, const double *p, int memspace,
                                double abstol, int maxiters, double step_threshold, double shrink_threshold,
                                double expand_threshold, double shrink_factor, double expand_factor, int max_shrink_times,
                                double *u_out, double *resid_out, int32_t *retcode_out, int32_t *iters_out);
int nk_batch_solve_trust_region_f32(nk_batch *B, int64_t nbatch, const float *u0, int u0_per_system, const float *p,
                                    int memspace, double abstol, int maxiters, double step_threshold, double shrink_threshold,
                                    double expand_threshold, double shrink_factor, double expand_factor, int max_shrink_times,
                                    float *u_out, float *resid_out, int32_t *retcode_out, int32_t *iters_out);
/* Jacobian-free methods (lib/SimpleNonlinearSolve/src/broyden.jl, klement.jl, dfsane.jl), one system per thread, n = 1..64
 * (registers while n <= 8, scratch above). Their kernels are a module of their own, compiled by hiprtc on the first call of
 * one of these entry points on an object and kept on it: nk_batch_create and the Newton kernels do not change. Common to
 * all three: AbsNormTerminationMode(maximum∘abs) on the NEW residual, right after it is evaluated (the Newton kernel checks
 * before its evaluation); a NaN residual never terminates; default abstol eps(T)^(4/5), maxiters 1000; resid = f(u) at the
 * returned u; retcodes NK_RET_SUCCESS / NK_RET_MAXITERS. Argument conventions as nk_batch_solve; real parameters <= 0
 * select the defaults; the _f32 twins take float arrays (scalars stay double and are rounded to float, T(x)).
 * SimpleBroyden (linesearch = nothing): iszero(f(u0)) ⇒ Success with iters 0; J⁻¹ = init_α·I with init_α = 1/alpha, or, for
 *   alpha <= 0 (`nothing`), max(‖u0‖₂, 1)/(2‖f(u0)‖₂) when ‖f(u0)‖₂ >= 1e-5, else 1; per iteration δx = −J⁻¹f_prev,
 *   u += δx, f, check, J⁻¹ += ((δx − J⁻¹δf)/(δx·J⁻¹δf)) (J⁻¹ᵀδx)ᵀ with no guard on a zero denominator.
 * SimpleKlement: diagonal J = 1 at start and wherever any entry is 0 (all reset); δx = f_prev ./ J, u −= δx, f, check,
 *   J += (f − f_prev − J·δ)/(δ²J² or 1e-5 where that is 0)·δ·J² with δ = −δx. No iszero shortcut.
 * For both, iters is the 1-based iteration that passed the check, or maxiters.
 * SimpleDFSane (η_k = f₁/k², the default eta_strategy): spectral steps d = −σ_k f with sign(σ)·clamp(|σ|, σ_min, σ_max)
 *   (NaN kept), the non-monotone line search against max of the last M merit values ‖f‖₂^n_exp (NaN propagates), step
 *   factors clamped to [τ_min, τ_max]·α. The counter k is the reference's: it counts outer iterations and inner line-search
 *   passes, both loops stop at k = maxiters (the last trial point is then taken and checked), and the merit value is stored
 *   in slot mod1(k, M). iters is k + 1 on Success (the iteration that passed the check) and maxiters otherwise, never more
 *   than maxiters. M is accepted in 1..32 and n_exp as 1 or 2; 0 selects the default (10, 2), any other value is
 *   NK_E_INVALID. Defaults σ_min = 1e-10, σ_max = 1e10, σ₁ = 1, γ = 1e-4, τ_min = 0.1, τ_max = 0.5.
 * Not offered: SimpleLimitedMemoryBroyden — its static (kernel) path keeps 2·threshold·n values (threshold 27) and, in its
 * unrolled first iterations, never advances xo (lbroyden.jl:256), a reference defect a port would have to copy or knowingly
 * diverge from; SimpleHalley — it needs second derivatives, and the reference leaves it out of its own kernel tests. */
int nk_batch_solve_broyden(nk_batch *B, int64_t nbatch, const double *u0, int u0_per_system, const double *p, int memspace,
                           double abstol, int maxiters, double alpha, double *u_out, double *resid_out, int32_t *retcode_out,
                           int32_t *iters_out);
int nk_batch_solve_broyden_f32(nk_batch *B, int64_t nbatch, const float *u0, int u0_per_system, const float *p, int memspace,
                               double abstol, int maxiters, double alpha, float *u_out, float *resid_out, int32_t *retcode_out,
                               int32_t *iters_out);
int nk_batch_solve_klement(nk_batch *B, int64_t nbatch, const double *u0, int u0_per_system, const double *p, int memspace,
                           double abstol, int maxiters, double *u_out, double *resid_out, int32_t *retcode_out,
                           int32_t *iters_out);
int nk_batch_solve_klement_f32(nk_batch *B, int64_t nbatch, const float *u0, int u0_per_system, const float *p, int memspace,
                               double abstol, int maxiters, float *u_out, float *resid_out, int32_t *retcode_out,
                               int32_t *iters_out);
int nk_batch_solve_dfsane(nk_batch *B, int64_t nbatch, const double *u0, int u0_per_system, const double *p, int memspace,
                          double abstol, int maxiters, double sigma_min, double sigma_max, double sigma_1, int M, double gamma,
                          double tau_min, double tau_max, int n_exp, double *u_out, double *resid_out, int32_t *retcode_out,
                          int32_t *iters_out);
int nk_batch_solve_dfsane_f32(nk_batch *B, int64_t nbatch, const float *u0, int u0_per_system, const float *p, int memspace,
                              double abstol, int maxiters, double sigma_min, double sigma_max, double sigma_1, int M,
                              double gamma, double tau_min, double tau_max, int n_exp, float *u_out, float *resid_out,
                              int32_t *retcode_out, int32_t *iters_out);
/* the Jacobian-free module's code object (nk_batch_broyden, nk_batch_klement, nk_batch_dfsane) for inspection, as
 * nk_batch_code_object; no device needed */
int nk_batch_jf_code_object(const char *source, int n, int nparams, int flags, void *buf, int64_t capacity, int64_t *bytes);

/* ---------------------------------------------------------------- ensembles of small nonlinear least-squares problems
 * m residuals, n unknowns, 1 <= n <= m <= 64, one problem per GPU thread: fitting a small model to each of many data sets.
 * SimpleGaussNewton — the reference's alias of SimpleNewtonRaphson (lib/SimpleNonlinearSolve/src/raphson.jl:31), declared on
 * Union{ImmutableNonlinearProblem, NonlinearLeastSquaresProblem} (raphson.jl:41-43) — and SimpleTrustRegion
 * (trust_region.jl:60-62). The source contract is that of nk_batch_create; only the output length differs:
 *     template <typename T> __device__ void nk_f(const T *u, const nk_real *p, T *f);   // u: n values, f: m values
 *     __device__ void nk_jac(const nk_real *u, const nk_real *p, nk_real *J);           // optional, row-major m×n
 * compiled with -DNK_N=n -DNK_M=m (nk_real = double, or float with NK_BATCH_FLOAT32); entries of f that the source does
 * not write are zero. Each fit's data travels in p (e.g. nparams = 2m for (x_i, y_i) pairs; nparams <= 256; p is read in
 * place when nparams > 32). m < n is NK_E_INVALID: the minimum-norm solution of an underdetermined problem is not offered.
 * m == n is accepted and runs the same kernels. These objects are a kind of their own: nk_batch_destroy frees them, the
 * square entry points (nk_batch_solve*) refuse them and the entry points below refuse square objects (NK_E_INVALID), as does
 * either precision's entry point on an object of the other.
 * Per problem:
 *  - termination is AbsNormTerminationMode(Base.Fix2(norm, 2)), the reference's :simple default for a
 *    NonlinearLeastSquaresProblem (lib/NonlinearSolveBase/src/termination_conditions.jl:381-383): ‖f‖₂ <= abstol, not
 *    max-abs; default abstol eps(T)^(4/5), maxiters 1000; a NaN norm never terminates. Consequence: a fit whose minimum
 *    residual is not zero never reports Success — it ends in NK_RET_MAXITERS (Gauss–Newton) or
 *    NK_RET_SHRINK_THRESHOLD_EXCEEDED / NK_RET_MAXITERS (trust region), as in the reference.
 *  - SimpleGaussNewton (raphson.jl:52-81): iszero(f(u0)) ⇒ Success with 0 iterations; per iteration δ = J \ f, u −= δ, the
 *    check on the residual of the previous iterate, then f and J at the new u.
 *  - SimpleTrustRegion (trust_region.jl:60-229, default radius update; the nlsolve_update_rule variant is not offered, as
 *    for the square kernel): a check before the loop, no iszero shortcut; H = JᵀJ (n×n), g = Jᵀf, dogleg with
 *    δN = −(J \ f); ratio, radius updates, defaults and retcodes as nk_batch_solve_trust_region;
 *    Δmax = max(‖f(u0)‖₂, max(u0) − min(u0)) over the n unknowns, Δ0 = Δmax/11.
 *  - J \ f is the least-squares solution by Householder QR with column pivoting, in place, with no normal equations.
 *    Divergence from the reference, which leaves rank deficiency to LAPACK's rank truncation: a column whose pivot has
 *    |r_kk| <= max(m, n)·eps(T)·|r_11| gets a zero step component (the basic solution, not the minimum-norm one). Column
 *    norms are taken without scaling, so entries beyond sqrt(floatmax(T)) overflow them.
 *  - resid_out is nbatch×m (f at the last evaluated iterate); the other outputs are as for nk_batch_solve.
 * Everything lives in registers while n <= 8 and m·(n + 2) <= 80 (Float64) or 128 (Float32) — e.g. 5×4, 8×3, 16×3, 8×8 in
 * both, 32×2 and 12×8 in Float32 only; found with the compiler's resource notes, not timed. Larger shapes run from scratch
 * memory. One problem per thread only: a per-wavefront form would need a
 * per-residual user function, a second source contract. */
int nk_batch_nlls_compile_check(const char *source, int n, int m, int nparams, int flags, int64_t *code_bytes);
/* the code object of the least-squares kernel set (nk_batch_gauss_newton, nk_batch_trust_region_nlls), as nk_batch_code_object */
int nk_batch_nlls_code_object(const char *source, int n, int m, int nparams, int flags, void *buf, int64_t capacity,
                              int64_t *bytes);
int nk_batch_create_nlls(nk_ctx *ctx, const char *source, int n, int m, int nparams, int flags, nk_batch **out);
int nk_batch_solve_gauss_newton(nk_batch *B, int64_t nbatch, const double *u0, int u0_per_system, const double *p, int memspace,
                                double abstol, int maxiters, double *u_out, double *resid_out, int32_t *retcode_out,
                                int32_t *iters_out);
int nk_batch_solve_gauss_newton_f32(nk_batch *B, int64_t nbatch, const float *u0, int u0_per_system, const float *p,
                                    int memspace, double abstol, int maxiters, float *u_out, float *resid_out,
                                    int32_t *retcode_out, int32_t *iters_out);
int nk_batch_solve_trust_region_nlls(nk_batch *B, int64_t nbatch, const double *u0, int u0_per_system, const double *p,
                                     int memspace, double abstol, int maxiters, double step_threshold, double shrink_threshold,
                                     double expand_threshold, double shrink_factor, double expand_factor, int max_shrink_times,
                                     double *u_out, double *resid_out, int32_t *retcode_out, int32_t *iters_out);
int nk_batch_solve_trust_region_nlls_f32(nk_batch *B, int64_t nbatch, const float *u0, int u0_per_system, const float *p,
                                         int memspace, double abstol, int maxiters, double step_threshold,
                                         double shrink_threshold, double expand_threshold, double shrink_factor,
                                         double expand_factor, int max_shrink_times, float *u_out, float *resid_out,
                                         int32_t *retcode_out, int32_t *iters_out);

/* ---------------------------------------------------------------- BLAS-1 building blocks (exported for
 * the bench / tests; all on the ctx stream, results of reductions are all-reduced over the ranks)
 *
 * The contract of these entry points and of nk_vec_axpby / nk_vec_fill:
 *  - Alignment: every vector (x, y, w, V) starts on a 16-byte boundary and ldv is even and at least n, so that every column of
 *    V does too. The kernels read pairs of doubles; a pointer that is only 8-byte aligned is not supported.
 *  - Edges: n = 0 is a no-op (a reduction returns 0) and may come with NULL vectors. n < 0 or nv < 0 is an error, as is
 *    nv > 64 (nk_multidot, nk_multiaxpy; nv = 0 is allowed there) and nv outside 1..32 (nk_fused_axpy_dot). An error launches
 *    nothing and leaves every vector as it was.
 *  - Zero coefficients (nk_vec_axpby, nk_axpy): a coefficient that is exactly zero, of either sign, means that its operand is
 *    not read: a = 0 gives y = b y whatever x holds (NaN and Inf included), b = 0 gives y = a x whatever y held, and
 *    a = b = 0 stores +0.0. Nonzero coefficients give a x + b y with one rounding per operation.
 *  - Aliasing: x may be the same pointer as y (y = a y + b y). Vectors that overlap in part are not allowed.
 *  - Overflow: nk_nrm2 is the unscaled sqrt(sum x_i^2): entries above about 1e154 overflow to Inf, entries below about 1e-154
 *    are lost. nk_norm_inf is exact; a NaN anywhere gives NaN.
 *  - Reductions are summed in a fixed order: the same call on the same data returns the same bits. */
int nk_dot(nk_ctx *ctx, int64_t n, const double *x, const double *y, double *result);
int nk_nrm2(nk_ctx *ctx, int64_t n, const double *x, double *result);
int nk_norm_inf(nk_ctx *ctx, int64_t n, const double *x, double *result);
int nk_axpy(nk_ctx *ctx, int64_t n, double a, const double *x, double *y);
/* Krylov basis kernels: V is column-major n × nv with leading dimension ldv (device).
 * h[j] = V[:,j]·w  and  w -= V h (returns ‖w‖² after the update in *wnorm2 if non-NULL). */
int nk_multidot(nk_ctx *ctx, int64_t n, int nv, const double *V, int64_t ldv, const double *w, double *h_host);
int nk_multiaxpy(nk_ctx *ctx, int64_t n, int nv, const double *V, int64_t ldv, const double *h_host,
                 double *w, double *wnorm2);
/* fused CGS2 pass on a lazily-normalised basis (v_j = s_j ṽ_j): w -= V (h∘s); h2[j] = s_j ṽ_j·w (j<nv), h2[nv] = ‖w‖² */
int nk_fused_axpy_dot(nk_ctx *ctx, int64_t n, int nv, const double *V, int64_t ldv, const double *h_host,
                      const double *s_host, double *w, double *h2_host);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_NK_H */
