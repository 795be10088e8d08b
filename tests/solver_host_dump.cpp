// Drives csrc/nk_linesearch.h and csrc/nk_termination.h on the host for tests/test_linesearch_host.py and
// tests/test_termination_host.py (built with g++, no device anywhere).
//
//   solver_host_dump ls <method> <function> <fail_at> [c1 rho_hi rho_lo maxiters order]
//     method: backtracking | static | strongwolfe | morethuente | hagerzhang (the method itself, given ϕ(0) and ϕ'(0) of the
//     function) or lsjl2 … lsjl5 (the dispatch on the method number, which evaluates ϕ(0), ϕ'(0) itself). The evaluator fails
//     with status 77 on its <fail_at>-th call (0: never). Prints "E <alpha> <want_dphi>" per evaluation, then
//     "R <status> <alpha> <failed>"; every double as a hex float.
//   solver_host_dump tc <mode> <abstol> <reltol> <patience_steps> <multiplier> <min_max_factor> <max_stalled_steps>
//                       <protective_threshold> <n_global>
//     reads "reset nf nfu relviol nf_inf u0_norm" / "check nf nfu relviol nf_inf step_norm" lines from stdin and answers each
//     with "<stop> <new_best> <retcode> <nsteps> <best_obj>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "nk_linesearch.h"
#include "nk_termination.h"

// ---- the scalar test functions: +, −, ×, ÷ only, in the expression order tests/test_linesearch_host.py repeats
typedef void (*phi_fn)(double a, double *p, double *d);
static void quartic(double k, double a, double *p, double *d) {  // ½((1 − kα)⁴ + 0.1α)
  const double t = 1.0 - k * a;
  *p = 0.5 * (t * t * t * t + 0.1 * a);
  *d = 0.5 * (0.1 - 4.0 * k * (t * t * t));
}
static void quad_bump(double k, double h, double s, double m, double a, double *p, double *d) {  // ½(1 − kα)² + h / (1 + s(α − m)²)
  const double t = 1.0 - k * a, e = a - m, q = 1.0 + s * (e * e);
  *p = 0.5 * (t * t) + h / q;
  *d = -(k * t) - (2.0 * h * s * e) / (q * q);
}
static void kink_bump(double mk, double h, double s, double m, double a, double *p, double *d) {  // 1 + |α − mk| + h / (1 + s(α − m)²)
  const double e = a - m, q = 1.0 + s * (e * e), b = h / q, db = (2.0 * h * s * e) / (q * q);
  if (a < mk) { *p = 1.0 + (mk - a) + b; *d = -1.0 - db; }
  else { *p = 1.0 + (a - mk) + b; *d = 1.0 - db; }
}
static void kink(double m, double a, double *p, double *d) {  // 1 + |α − m|
  if (a < m) { *p = 1.0 + (m - a); *d = -1.0; }
  else { *p = 1.0 + (a - m); *d = 1.0; }
}
static void vee(double m, double sl, double sr, double a, double *p, double *d) {
  if (a < m) { *p = 1.0 + sl * (m - a); *d = -sl; }
  else { *p = 1.0 + sr * (a - m); *d = sr; }
}
static void f_step_up(double a, double *p, double *d) {
  if (a > 0.3) { *p = 3.0 - a; *d = -1.0; }
  else { *p = 1.0 - a; *d = -1.0; }
}
static void f_nan_slope(double a, double *p, double *d) {
  if (a > 0.9) { *p = 3.0 - a; *d = -1.0; }
  else if (a > 0.6) { *p = 0.4 + (a - 0.6); *d = 1.0; }
  else if (a > 0.4) { *p = 1.0 - a; *d = NAN; }
  else { *p = 1.0 - a; *d = -1.0; }
}
static void f_flat_kink(double a, double *p, double *d) {
  *p = 1.0;
  if (a == 0.0) *d = -0.001 * 1e-18;
  else if (a < 0.3) *d = -(1e-18 * (1.0 + a));
  else *d = 1e-18;
}
static void f_steep_wall(double a, double *p, double *d) {
  if (a > 10.0) { *p = 2.0; *d = 1e308; }
  else { *p = 1.0 - 0.01 * a; *d = -0.01; }
}
static void cliff(phi_fn base, double at, double value, double a, double *p, double *d) {
  if (a > at) { *p = value; *d = value; }
  else base(a, p, d);
}
static void f_quartic_full(double a, double *p, double *d) { quartic(0.9, a, p, d); }
static void f_quartic_inside(double a, double *p, double *d) { quartic(3.0, a, p, d); }
static void f_quartic_tiny(double a, double *p, double *d) { quartic(1000.0, a, p, d); }
static void f_linear_down(double a, double *p, double *d) { *p = 1.0 - a; *d = -1.0; }
static void f_recip(double a, double *p, double *d) { *p = 1.0 / (1.0 + a); *d = -1.0 / ((1.0 + a) * (1.0 + a)); }
static void f_rising(double a, double *p, double *d) { *p = 0.5 * ((1.0 + a) * (1.0 + a)); *d = 1.0 + a; }
static void f_quad_bump(double a, double *p, double *d) { quad_bump(1.6, 0.8, 200.0, 0.6, a, p, d); }
static void f_kink_bump(double a, double *p, double *d) { kink_bump(0.3, 0.005, 400.0, 0.7, a, p, d); }
static void f_kink(double a, double *p, double *d) { kink(0.3, a, p, d); }
static void f_kink_tiny(double a, double *p, double *d) { kink(1e-20, a, p, d); }
static void f_kink_far(double a, double *p, double *d) { kink(40000.0, a, p, d); }
static void f_cliff_inf(double a, double *p, double *d) { cliff(f_quartic_inside, 0.3, INFINITY, a, p, d); }
static void f_cliff_nan(double a, double *p, double *d) { cliff(f_quartic_inside, 0.3, NAN, a, p, d); }
static void f_recip_cliff_inf(double a, double *p, double *d) { cliff(f_recip, 0.3, INFINITY, a, p, d); }
static void f_recip_cliff_nan(double a, double *p, double *d) { cliff(f_recip, 0.125, NAN, a, p, d); }
static void f_recip_cliff_adjacent(double a, double *p, double *d) { cliff(f_recip, 0x1.1cd4a1da6fa5ep-2, INFINITY, a, p, d); }
static void f_vee(double a, double *p, double *d) { vee(0.6, 1.0, 1.2, a, p, d); }
static void f_nan_beyond_zero(double a, double *p, double *d) { cliff(f_linear_down, 0.0, NAN, a, p, d); }
static void f_inf_beyond_zero(double a, double *p, double *d) { cliff(f_linear_down, 0.0, INFINITY, a, p, d); }

static const struct { const char *name; phi_fn fn; } FUNCTIONS[] = {
    {"quartic_full", f_quartic_full}, {"quartic_inside", f_quartic_inside}, {"quartic_tiny", f_quartic_tiny},
    {"linear_down", f_linear_down}, {"recip", f_recip}, {"rising", f_rising}, {"quad_bump", f_quad_bump},
    {"kink_bump", f_kink_bump}, {"kink", f_kink}, {"kink_tiny", f_kink_tiny}, {"kink_far", f_kink_far}, {"cliff_inf", f_cliff_inf},
    {"cliff_nan", f_cliff_nan}, {"recip_cliff_inf", f_recip_cliff_inf}, {"recip_cliff_nan", f_recip_cliff_nan},
    {"recip_cliff_adjacent", f_recip_cliff_adjacent}, {"vee", f_vee}, {"step_up", f_step_up}, {"nan_slope", f_nan_slope},
    {"flat_kink", f_flat_kink}, {"steep_wall", f_steep_wall},
    {"nan_beyond_zero", f_nan_beyond_zero}, {"inf_beyond_zero", f_inf_beyond_zero}};

static int run_ls(int argc, char **argv) {
  if (argc < 5) return 2;
  const std::string method = argv[2];
  phi_fn fn = nullptr;
  for (const auto &f : FUNCTIONS)
    if (!strcmp(f.name, argv[3])) fn = f.fn;
  if (!fn) { fprintf(stderr, "no function %s\n", argv[3]); return 2; }
  const int fail_at = atoi(argv[4]);
  int calls = 0;
  const auto eval = [&](double a, double *p, double *d) {
    printf("E %a %d\n", a, d ? 1 : 0);
    if (++calls == fail_at) return 77;
    double dd;
    fn(a, p, d ? d : &dd);
    return 0;
  };
  double phi0, dphi0, alpha = -1.0;
  bool failed = false;
  fn(0.0, &phi0, &dphi0);
  int rc = 2;
  if (method == "backtracking") {
    if (argc < 10) return 2;
    rc = ls_backtracking(eval, phi0, dphi0, strtod(argv[5], nullptr), strtod(argv[6], nullptr), strtod(argv[7], nullptr),
                         atoi(argv[8]), atoi(argv[9]), &alpha, &failed);
  } else if (method == "static") rc = ls_static(eval, &alpha);
  else if (method == "strongwolfe") rc = ls_strongwolfe(eval, phi0, dphi0, &alpha);
  else if (method == "morethuente") rc = ls_morethuente(eval, phi0, dphi0, &alpha);
  else if (method == "hagerzhang") rc = ls_hagerzhang(eval, phi0, dphi0, &alpha, &failed);
  else if (method.rfind("lsjl", 0) == 0) rc = ls_lsjl(eval, atoi(method.c_str() + 4), &alpha, &failed);
  else { fprintf(stderr, "no method %s\n", method.c_str()); return 2; }
  printf("R %d %a %d\n", rc, alpha, failed ? 1 : 0);
  return 0;
}

static int run_tc(int argc, char **argv) {
  if (argc < 11) return 2;
  tc_config c;
  c.mode = atoi(argv[2]);
  c.abstol = strtod(argv[3], nullptr);
  c.reltol = strtod(argv[4], nullptr);
  c.patience_steps = atoi(argv[5]);
  c.patience_objective_multiplier = strtod(argv[6], nullptr);
  c.min_max_factor = strtod(argv[7], nullptr);
  c.max_stalled_steps = atoi(argv[8]);
  c.protective_threshold = strtod(argv[9], nullptr);
  c.n_global = atoll(argv[10]);
  tc_state s;
  char what[16], x[5][64];
  while (scanf("%15s %63s %63s %63s %63s %63s", what, x[0], x[1], x[2], x[3], x[4]) == 6) {
    tc_quant q;
    q.nf = strtod(x[0], nullptr); q.nfu = strtod(x[1], nullptr); q.relviol = strtod(x[2], nullptr); q.nf_inf = strtod(x[3], nullptr);
    const double last = strtod(x[4], nullptr);
    tc_verdict v{false, false};
    if (!strcmp(what, "reset")) tc_reset(c, s, q, last);
    else v = tc_check(c, s, q, last);
    printf("%d %d %d %d %a\n", v.stop ? 1 : 0, v.new_best ? 1 : 0, s.retcode, s.nsteps, s.best_obj);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 2 && !strcmp(argv[1], "ls")) return run_ls(argc, argv);
  if (argc >= 2 && !strcmp(argv[1], "tc")) return run_tc(argc, argv);
  fprintf(stderr, "usage: solver_host_dump ls|tc …\n");
  return 2;
}
