// The termination cache as plain host arithmetic: the nine SciMLBase termination modes (termination_conditions.jl:243-376),
// two norms, the patience test, the stall test, the protective threshold and the best objective. The solver driver reduces the
// current (fu, u) to a tc_quant on the device and acts on the verdict (it keeps the best iterate, it rolls back to it); what is
// here sees a handful of doubles and two ring buffers, so a host compiler builds it and tests/test_termination_host.py walks it
// against oracle/reference_restatement.py::TerminationCache.
#pragma once

#include <math.h>
#include <stdint.h>

#include <vector>

#include "mi355x_nk.h"

enum {
  TM_ABSNORM_SAFEBEST = 0,  // default_termination_mode(::NonlinearProblem, Val(:regular))  (:385-389)
  TM_NORM = 1, TM_REL = 2, TM_RELNORM = 3, TM_RELNORM_SAFE = 4, TM_RELNORM_SAFEBEST = 5,
  TM_ABS = 6, TM_ABSNORM = 7, TM_ABSNORM_SAFE = 8
};
inline bool tm_safe(int m) { return m == TM_ABSNORM_SAFEBEST || m == TM_ABSNORM_SAFE || m == TM_RELNORM_SAFE || m == TM_RELNORM_SAFEBEST; }
inline bool tm_best(int m) { return m == TM_ABSNORM_SAFEBEST || m == TM_RELNORM_SAFEBEST; }
inline bool tm_rel(int m) { return m == TM_RELNORM_SAFE || m == TM_RELNORM_SAFEBEST; }
inline bool tm_needs_pair(int m) { return m == TM_NORM || m == TM_REL || m == TM_RELNORM || tm_rel(m); }

struct tc_config {
  int mode = TM_ABSNORM_SAFEBEST;
  double abstol = 0, reltol = 0;
  int patience_steps = 100;
  double patience_objective_multiplier = 3.0, min_max_factor = 1.3;
  int max_stalled_steps = 32;        // < 0: no stall test
  double protective_threshold = 0;   // ≤ 0: off
  int64_t n_global = 0;
};
struct tc_state {
  int retcode = NK_RET_DEFAULT, nsteps = 0;
  double initial_obj = 0, best_obj = 0;
  double u0_norm = 0;  // ‖u0‖₂ for the relative stall test
  std::vector<double> objectives_trace, step_norm_trace;
};
struct tc_quant {
  double nf = 0;      // internalnorm(fu)
  double nfu = 0;     // internalnorm(fu .+ u)
  double relviol = 0; // max_i(|fu_i| − reltol |u_i + fu_i|)  (RelTerminationMode: converged iff ≤ 0)
  double nf_inf = 0;  // ‖fu‖∞ (AbsTerminationMode, whatever the internalnorm)
};
struct tc_verdict {
  bool stop;      // the solve must end: the reason is tc_state.retcode
  bool new_best;  // the current iterate is the best one so far (only the *Best modes)
};

inline double tc_objective(const tc_config &c, const tc_quant &q) {
  if (tm_rel(c.mode)) return q.nf / (q.nfu + 2.220446049250313e-16 * c.reltol);  // eps(reltol)
  return q.nf;
}

// (re)initialisation; q: the quantities at u0, u0_norm: ‖u0‖₂ (read only by the relative stall test)
inline void tc_reset(const tc_config &c, tc_state &s, const tc_quant &q, double u0_norm) {
  s.retcode = NK_RET_DEFAULT;
  s.nsteps = 0;
  s.initial_obj = tm_safe(c.mode) ? tc_objective(c, q) : INFINITY;
  s.best_obj = s.initial_obj;
  s.objectives_trace.assign(c.patience_steps > 0 ? c.patience_steps : 1, 0.0);
  if (c.max_stalled_steps >= 0) s.step_norm_trace.assign(c.max_stalled_steps > 0 ? c.max_stalled_steps : 1, 0.0);
  else s.step_norm_trace.clear();
  s.u0_norm = u0_norm;
}
// q: the quantities at the current (fu, u); step_norm = ‖u − uprev‖₂
inline tc_verdict tc_check(const tc_config &c, tc_state &s, const tc_quant &q, double step_norm) {
  const int mode = c.mode;
  if (!tm_safe(mode)) {  // plain modes: check_convergence only (termination_conditions.jl:232-241)
    bool conv = false;
    switch (mode) {
      case TM_NORM: conv = (q.nf <= c.abstol) || (q.nf <= c.reltol * q.nfu); break;
      case TM_REL: conv = (q.relviol <= 0.0); break;
      case TM_RELNORM: conv = (q.nf <= c.reltol * q.nfu); break;
      case TM_ABS: conv = (q.nf_inf <= c.abstol); break;
      case TM_ABSNORM: conv = (q.nf <= c.abstol); break;
      default: break;
    }
    if (conv) s.retcode = NK_RET_SUCCESS;
    return {conv, false};
  }
  const double objective = tc_objective(c, q);
  const double criteria = tm_rel(mode) ? c.reltol : c.abstol;
  if (!isfinite(objective)) { s.retcode = NK_RET_UNSTABLE; return {true, false}; }
  if (c.protective_threshold > 0.0 && objective > s.initial_obj * c.protective_threshold * (double)c.n_global) {
    s.retcode = NK_RET_UNSTABLE;
    return {true, false};
  }
  bool new_best = false;
  if (tm_best(mode) && objective < s.best_obj) {
    s.best_obj = objective;
    new_best = true;
  }
  if (objective <= criteria) { s.retcode = NK_RET_SUCCESS; return {true, new_best}; }
  s.nsteps += 1;
  const int L = (int)s.objectives_trace.size();
  s.objectives_trace[(s.nsteps - 1) % L] = objective;
  if (objective <= c.patience_objective_multiplier * criteria && s.nsteps > c.patience_steps) {
    const int cnt = s.nsteps < L ? s.nsteps : L;
    double mn = INFINITY, mx = -INFINITY;
    for (int i = 0; i < cnt; ++i) { mn = fmin(mn, s.objectives_trace[i]); mx = fmax(mx, s.objectives_trace[i]); }
    if (mn < c.min_max_factor * mx) { s.retcode = NK_RET_STALLED; return {true, new_best}; }
  }
  if (!s.step_norm_trace.empty()) {
    const int L2 = (int)s.step_norm_trace.size();
    s.step_norm_trace[(s.nsteps - 1) % L2] = step_norm;
    if (s.nsteps > c.max_stalled_steps) {
      double mx = -INFINITY;
      for (double v : s.step_norm_trace) mx = fmax(mx, v);
      const bool stalled = tm_rel(mode) ? (mx <= c.reltol * (mx + s.u0_norm)) : (mx <= c.abstol);
      if (stalled) { s.retcode = NK_RET_STALLED; return {true, new_best}; }
    }
  }
  s.retcode = NK_RET_FAILURE;
  return {false, new_best};
}
