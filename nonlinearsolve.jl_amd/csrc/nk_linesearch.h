// The line searches of the first-order step as plain host arithmetic on ϕ(α) = ½‖f(u + α δu)‖² and ϕ'(α): BackTracking and
// LineSearchesJL(; method = Static | StrongWolfe | MoreThuente | HagerZhang). A method sees the problem only through ONE
// evaluator, a callable
//     int eval(double alpha, double *phi, double *dphi)      (dphi == nullptr: ϕ only; a non-zero return is an error)
// and decides from a handful of doubles what to evaluate next; an evaluator's error is returned at once, as it is. Which α is
// requested, with or without ϕ', in which order — the evaluations that look redundant included — is the contract
// (tests/test_linesearch_host.py holds it, bit for bit, against oracle/reference_restatement.py). Nothing here touches the
// device: the solver driver supplies the evaluator (one residual at the trial point, for ϕ' one Jacobian-vector product there, one
// fused reduction, one fetch) and, for BackTracking, ϕ(0) and ϕ'(0).
#pragma once

#include <math.h>

#include <vector>

constexpr int LS_BAD_METHOD = 1;  // ls_lsjl: no such method (not a status an evaluator returns)

#define LS_TRY(expr) do { const int ls_rc_ = (expr); if (ls_rc_ != 0) return ls_rc_; } while (0)

// ---- BackTracking line search on ϕ(α) = ½‖f(u + α δu)‖² (LineSearches.jl BackTracking restated, [EXT]):
// sufficient decrease ϕ(α) ≤ ϕ(0) + c₁ α ϕ'(0); quadratic, then cubic interpolation, safeguarded to
// [ρ_lo α, ρ_hi α]. Every ϕ evaluation is one residual (stats.nf += 1, as the reference's line-search cache does).
template <class Eval> int ls_backtracking(Eval &&eval, double phi0, double dphi0, double c1, double rho_hi, double rho_lo,
                                          int maxiters, int order, double *alpha_out, bool *failed) {
  *failed = false;
  double a1 = 1.0, a2 = 1.0, phx0 = phi0, phx1 = phi0;
  LS_TRY(eval(a1, &phx1, nullptr));
  int iterfinite = 0;
  const int iterfinitemax = 1074;  // -log2(eps(Float64)) style bound used by LineSearches.jl
  while (!isfinite(phx1) && iterfinite < iterfinitemax) {
    ++iterfinite;
    a1 = a2;
    a2 = a1 / 2.0;
    LS_TRY(eval(a2, &phx1, nullptr));
  }
  int iteration = 0;
  while (phx1 > phi0 + c1 * a2 * dphi0) {
    ++iteration;
    if (iteration > maxiters) { *failed = true; break; }
    double atmp;
    if (order == 2 || iteration == 1) {
      atmp = -(dphi0 * a2 * a2) / (2.0 * (phx1 - phi0 - dphi0 * a2));
    } else {
      const double div = 1.0 / (a1 * a1 * a2 * a2 * (a2 - a1));
      const double ca = (a1 * a1 * (phx1 - phi0 - dphi0 * a2) - a2 * a2 * (phx0 - phi0 - dphi0 * a1)) * div;
      const double cb = (-a1 * a1 * a1 * (phx1 - phi0 - dphi0 * a2) + a2 * a2 * a2 * (phx0 - phi0 - dphi0 * a1)) * div;
      if (fabs(ca) <= 2.220446049250313e-16) atmp = dphi0 / (2.0 * cb);  // isapprox(a, 0; atol = eps)
      else {
        const double disc = fmax(cb * cb - 3.0 * ca * dphi0, 0.0);
        atmp = (-cb + sqrt(disc)) / (3.0 * ca);
      }
    }
    a1 = a2;
    atmp = (atmp == atmp) ? fmin(atmp, a2 * rho_hi) : a2 * rho_hi;  // NaNMath.min
    a2 = (atmp == atmp) ? fmax(atmp, a2 * rho_lo) : a2 * rho_lo;    // NaNMath.max
    phx0 = phx1;
    LS_TRY(eval(a2, &phx1, nullptr));
  }
  *alpha_out = a2;
  return 0;
}

// ---- LineSearchesJL(; method = Static | StrongWolfe | MoreThuente | HagerZhang) [EXT: LineSearch.jl's wrapper around LineSearches.jl,
// the methods of lib/NonlinearSolveFirstOrder/test/rootfind_tests__item2.jl:40-46] on ϕ(α) = ½‖f(u + α δu)‖²,
// ϕ'(α) = f(u + α δu)ᵀ J(u + α δu) δu. Restated from the published algorithms with LineSearches.jl's default parameters
// (oracle/reference_restatement.py::_lsjl is the same code in Python; its Moré–Thuente step function is pinned against SciPy's
// MINPACK-2 dcstep).
// LineSearches.Static: the proposed step, halved while ϕ is not finite
template <class Eval> int ls_static(Eval &&eval, double *alpha) {
  double a = 1.0, pa;
  LS_TRY(eval(a, &pa, nullptr));
  for (int it = 0; !isfinite(pa) && it < 52; ++it) {
    a /= 2.0;
    LS_TRY(eval(a, &pa, nullptr));
  }
  *alpha = a;
  return 0;
}
// LineSearches.StrongWolfe (Nocedal & Wright alg. 3.5 / 3.6, cubic interpolation, c₁ = 1e-4, c₂ = 0.9, ρ = 2)
inline double ls_sw_interp(double a1, double a2, double p1, double p2, double d1, double d2) {
  const double q1 = d1 + d2 - 3.0 * (p1 - p2) / (a1 - a2);
  const double rad = q1 * q1 - d1 * d2;
  const double q2 = rad >= 0.0 ? sqrt(rad) : NAN;
  return a2 - (a2 - a1) * ((d2 + q2 - q1) / (d2 - d1 + 2.0 * q2));
}
template <class Eval> int ls_sw_zoom(Eval &&eval, double alo, double ahi, double phi0, double dphi0, double *out) {
  const double c1 = 1e-4, c2 = 0.9;
  double aj = NAN;
  for (int it = 0; it < 10; ++it) {
    double plo, dlo, phi_, dhi, pj, dj;
    LS_TRY(eval(alo, &plo, &dlo));
    LS_TRY(eval(ahi, &phi_, &dhi));
    aj = (alo < ahi) ? ls_sw_interp(alo, ahi, plo, phi_, dlo, dhi) : ls_sw_interp(ahi, alo, phi_, plo, dhi, dlo);
    LS_TRY(eval(aj, &pj, nullptr));
    if (pj > phi0 + c1 * aj * dphi0 || pj > plo) {
      ahi = aj;
    } else {
      LS_TRY(eval(aj, &pj, &dj));
      if (fabs(dj) <= -c2 * dphi0) break;
      if (dj * (ahi - alo) >= 0.0) ahi = alo;
      alo = aj;
    }
  }
  *out = aj;
  return 0;
}
template <class Eval> int ls_strongwolfe(Eval &&eval, double phi0, double dphi0, double *alpha) {
  const double c1 = 1e-4, c2 = 0.9, rho = 2.0, a_max = 65536.0;
  double a_prev = 0.0, a_i = 1.0, p_prev = phi0, p_i, d_i, tmp;
  for (int i = 1; a_i < a_max; ++i) {
    LS_TRY(eval(a_i, &p_i, nullptr));
    if (p_i > phi0 + c1 * a_i * dphi0 || (p_i >= p_prev && i > 1)) {
      LS_TRY(ls_sw_zoom(eval, a_prev, a_i, phi0, dphi0, alpha));
      return eval(*alpha, &tmp, nullptr);  // the method returns (α*, ϕ(α*)): one more evaluation
    }
    LS_TRY(eval(a_i, &p_i, &d_i));
    if (fabs(d_i) <= -c2 * dphi0) { *alpha = a_i; return 0; }
    if (d_i >= 0.0) {
      LS_TRY(ls_sw_zoom(eval, a_i, a_prev, phi0, dphi0, alpha));
      return eval(*alpha, &tmp, nullptr);
    }
    a_prev = a_i;
    p_prev = p_i;
    a_i *= rho;
  }
  *alpha = a_max;
  return eval(a_max, &tmp, nullptr);
}
// MINPACK cstep (Moré & Thuente 1994): safeguarded cubic / quadratic step + update of the interval of uncertainty
struct mt_state { double stx, fx, dgx, sty, fy, dgy, alpha, f, dg; bool bracketed; int info; };
inline void ls_cstep(mt_state &m, double amin, double amax) {
  double &stx = m.stx, &fx = m.fx, &dgx = m.dgx, &sty = m.sty, &fy = m.fy, &dgy = m.dgy, &alpha = m.alpha;
  const double f = m.f, dg = m.dg;
  m.info = 0;
  if ((m.bracketed && (alpha <= fmin(stx, sty) || alpha >= fmax(stx, sty))) || dgx * (alpha - stx) >= 0.0 || amax < amin) return;
  const double sgnd = dg * (dgx / fabs(dgx));
  bool bound;
  double af;
  if (f > fx) {
    m.info = 1; bound = true;
    const double theta = 3.0 * (fx - f) / (alpha - stx) + dgx + dg;
    const double sc = fmax(fabs(theta), fmax(fabs(dgx), fabs(dg)));
    double gamma = sc * sqrt((theta / sc) * (theta / sc) - (dgx / sc) * (dg / sc));
    if (alpha < stx) gamma = -gamma;
    const double pp = gamma - dgx + theta, q = gamma - dgx + gamma + dg, r = pp / q;
    const double ac = stx + r * (alpha - stx);
    const double aq = stx + ((dgx / ((fx - f) / (alpha - stx) + dgx)) / 2.0) * (alpha - stx);
    af = (fabs(ac - stx) < fabs(aq - stx)) ? ac : (ac + aq) / 2.0;
    m.bracketed = true;
  } else if (sgnd < 0.0) {
    m.info = 2; bound = false;
    const double theta = 3.0 * (fx - f) / (alpha - stx) + dgx + dg;
    const double sc = fmax(fabs(theta), fmax(fabs(dgx), fabs(dg)));
    double gamma = sc * sqrt((theta / sc) * (theta / sc) - (dgx / sc) * (dg / sc));
    if (alpha > stx) gamma = -gamma;
    const double pp = gamma - dg + theta, q = gamma - dg + gamma + dgx, r = pp / q;
    const double ac = alpha + r * (stx - alpha);
    const double aq = alpha + (dg / (dg - dgx)) * (stx - alpha);
    af = (fabs(ac - alpha) > fabs(aq - alpha)) ? ac : aq;
    m.bracketed = true;
  } else if (fabs(dg) < fabs(dgx)) {
    m.info = 3; bound = true;
    const double theta = 3.0 * (fx - f) / (alpha - stx) + dgx + dg;
    const double sc = fmax(fabs(theta), fmax(fabs(dgx), fabs(dg)));
    double gamma = sc * sqrt(fmax(0.0, (theta / sc) * (theta / sc) - (dgx / sc) * (dg / sc)));
    if (alpha > stx) gamma = -gamma;
    const double pp = gamma - dg + theta, q = gamma + dgx - dg + gamma, r = pp / q;
    double ac;
    if (r < 0.0 && gamma != 0.0) ac = alpha + r * (stx - alpha);
    else if (alpha > stx) ac = amax;
    else ac = amin;
    const double aq = alpha + (dg / (dg - dgx)) * (stx - alpha);
    if (m.bracketed) af = (fabs(alpha - ac) < fabs(alpha - aq)) ? ac : aq;
    else af = (fabs(alpha - ac) > fabs(alpha - aq)) ? ac : aq;
  } else {
    m.info = 4; bound = false;
    if (m.bracketed) {
      const double theta = 3.0 * (f - fy) / (sty - alpha) + dgy + dg;
      const double sc = fmax(fabs(theta), fmax(fabs(dgy), fabs(dg)));
      double gamma = sc * sqrt((theta / sc) * (theta / sc) - (dgy / sc) * (dg / sc));
      if (alpha > sty) gamma = -gamma;
      const double pp = gamma - dg + theta, q = gamma - dg + gamma + dgy, r = pp / q;
      af = alpha + r * (sty - alpha);
    } else if (alpha > stx) af = amax;
    else af = amin;
  }
  if (f > fx) { sty = alpha; fy = f; dgy = dg; }
  else {
    if (sgnd < 0.0) { sty = stx; fy = fx; dgy = dgx; }
    stx = alpha; fx = f; dgx = dg;
  }
  af = fmax(amin, fmin(amax, af));
  alpha = af;
  if (m.bracketed && bound) {
    if (sty > stx) alpha = fmin(stx + (2.0 / 3.0) * (sty - stx), alpha);
    else alpha = fmax(stx + (2.0 / 3.0) * (sty - stx), alpha);
  }
}
// LineSearches.MoreThuente (f_tol = 1e-4, gtol = 0.9, x_tol = 1e-8, alphamin = 1e-16, alphamax = 65536, maxfev = 100)
template <class Eval> int ls_morethuente(Eval &&eval, double phi0, double dphi0, double *alpha_out) {
  const double f_tol = 1e-4, gtol = 0.9, x_tol = 1e-8, amin = 1e-16, amax = 65536.0;
  const int maxfev = 100;
  int info = 0, info_cstep = 1, nfev = 0;
  bool stage1 = true;
  const double finit = phi0, dgtest = f_tol * dphi0;
  double width = amax - amin, width1 = 2.0 * width;
  mt_state m;
  m.stx = 0.0; m.fx = finit; m.dgx = dphi0;
  m.sty = 0.0; m.fy = finit; m.dgy = dphi0;
  m.bracketed = false;
  m.info = 1;
  double alpha = fmin(fmax(1.0, amin), amax), f, dg, stmin, stmax;
  LS_TRY(eval(alpha, &f, &dg));
  nfev++;
  for (int itf = 0; (!isfinite(f) || !isfinite(dg)) && itf < 52; ++itf) {
    alpha /= 2.0;
    LS_TRY(eval(alpha, &f, &dg));
    nfev++;
    m.stx = 0.875 * alpha;
  }
  for (;;) {
    if (m.bracketed) { stmin = fmin(m.stx, m.sty); stmax = fmax(m.stx, m.sty); }
    else { stmin = m.stx; stmax = alpha + 4.0 * (alpha - m.stx); }
    stmin = fmax(amin, stmin);
    stmax = fmin(amax, stmax);
    alpha = fmin(fmax(alpha, amin), amax);
    if ((m.bracketed && (alpha <= stmin || alpha >= stmax)) || nfev >= maxfev - 1 || info_cstep == 0 ||
        (m.bracketed && stmax - stmin <= x_tol * stmax))
      alpha = m.stx;
    LS_TRY(eval(alpha, &f, &dg));  // (the first pass evaluates the initial step a second time, as LineSearches.jl does)
    nfev++;
    const double ftest1 = finit + alpha * dgtest;
    if ((m.bracketed && (alpha <= stmin || alpha >= stmax)) || info_cstep == 0) info = 6;
    if (alpha == amax && f <= ftest1 && dg <= dgtest) info = 5;
    if (alpha == amin && (f > ftest1 || dg >= dgtest)) info = 4;
    if (nfev >= maxfev) info = 3;
    if (m.bracketed && stmax - stmin <= x_tol * stmax) info = 2;
    if (f <= ftest1 && fabs(dg) <= -gtol * dphi0) info = 1;
    if (info != 0) break;
    if (stage1 && f <= ftest1 && dg >= fmin(f_tol, gtol) * dphi0) stage1 = false;
    m.alpha = alpha;
    if (stage1 && f <= m.fx && f > ftest1) {  // the modified function ψ(α) = ϕ(α) − ϕ(0) − f_tol ϕ'(0) α
      mt_state mm = m;
      mm.fx = m.fx - m.stx * dgtest; mm.fy = m.fy - m.sty * dgtest; mm.f = f - alpha * dgtest;
      mm.dgx = m.dgx - dgtest; mm.dgy = m.dgy - dgtest; mm.dg = dg - dgtest;
      ls_cstep(mm, stmin, stmax);
      m.stx = mm.stx; m.sty = mm.sty; m.alpha = mm.alpha; m.bracketed = mm.bracketed; m.info = mm.info;
      m.fx = mm.fx + mm.stx * dgtest; m.fy = mm.fy + mm.sty * dgtest;
      m.dgx = mm.dgx + dgtest; m.dgy = mm.dgy + dgtest;
    } else {
      m.f = f; m.dg = dg;
      ls_cstep(m, stmin, stmax);
    }
    alpha = m.alpha;
    info_cstep = m.info;
    if (m.bracketed) {
      if (fabs(m.sty - m.stx) >= (2.0 / 3.0) * width1) alpha = m.stx + (m.sty - m.stx) / 2.0;
      width1 = width;
      width = fabs(m.sty - m.stx);
    }
  }
  *alpha_out = alpha;
  return 0;
}
// LineSearches.HagerZhang (Hager & Zhang 2005: bracket B0–B3, secant² S1–S4, update U0–U3 with bisection θ = ½, Wolfe /
// approximate Wolfe tests; δ = 0.1, σ = 0.9, ρ = 5, ε = 1e-6, γ = 0.66, ≤ 50 iterations, ψ₃ = 0.1). The method's exceptions
// (non-descent direction, iteration limit, lost bracket) are reported as a failed line search at the best step so far.
struct hz_state {
  std::vector<double> a, v, d;  // step lengths, ϕ, ϕ′ of every evaluation (index 0: α = 0)
  double phi_0, dphi_0, phi_lim;
  bool lost = false;
};
template <class Eval> int hz_eval(Eval &&eval, hz_state &h, double alpha, double *p, double *dp) {
  LS_TRY(eval(alpha, p, dp));
  h.a.push_back(alpha); h.v.push_back(*p); h.d.push_back(*dp);
  return 0;
}
inline bool hz_wolfe(const hz_state &h, double c, double pc, double dc) {
  const double delta = 0.1, sigma = 0.9;
  const bool w1 = delta * h.dphi_0 >= (pc - h.phi_0) / c && dc >= sigma * h.dphi_0;
  const bool w2 = (2.0 * delta - 1.0) * h.dphi_0 >= dc && dc >= sigma * h.dphi_0 && pc <= h.phi_lim;
  return w1 || w2;
}
template <class Eval> int hz_bisect(Eval &&eval, hz_state &h, int *ia, int *ib) {
  double a = h.a[*ia], b = h.a[*ib];
  while (b - a > nextafter(b, INFINITY) - b) {
    const double dd = (a + b) / 2.0;
    double pd, gd;
    LS_TRY(hz_eval(eval, h, dd, &pd, &gd));
    const int id = (int)h.a.size() - 1;
    if (gd >= 0.0) { *ib = id; return 0; }
    if (pd <= h.phi_lim) { a = dd; *ia = id; }
    else { b = dd; *ib = id; }
  }
  return 0;
}
template <class Eval> int hz_update(Eval &&eval, hz_state &h, int ia, int ib, int ic, int *oa, int *ob) {
  const double a = h.a[ia], b = h.a[ib], c = h.a[ic];
  *oa = ia; *ob = ib;
  if (c < a || c > b) return 0;
  if (h.d[ic] >= 0.0) { *ob = ic; return 0; }
  if (h.v[ic] <= h.phi_lim) { *oa = ic; return 0; }
  *ob = ic;
  return hz_bisect(eval, h, oa, ob);
}
inline double hz_secant(double a, double b, double da, double db) { return (a * db - b * da) / (db - da); }
template <class Eval> int hz_secant2(Eval &&eval, hz_state &h, int ia, int ib, bool *iswolfe, int *oA, int *oB) {
  const double a0 = h.a[ia], b0 = h.a[ib], da = h.d[ia], db = h.d[ib];
  *iswolfe = false;
  if (!(da < 0.0 && db >= 0.0)) { h.lost = true; *oA = ia; *oB = ib; return 0; }
  double c = hz_secant(a0, b0, da, db), pc, dc;
  LS_TRY(hz_eval(eval, h, c, &pc, &dc));
  int ic = (int)h.a.size() - 1;
  if (hz_wolfe(h, c, pc, dc)) { *iswolfe = true; *oA = *oB = ic; return 0; }
  int iA, iB;
  LS_TRY(hz_update(eval, h, ia, ib, ic, &iA, &iB));
  const double a = h.a[iA], b = h.a[iB];
  if (iB == ic) c = hz_secant(h.a[ib], h.a[iB], h.d[ib], h.d[iB]);
  else if (iA == ic) c = hz_secant(h.a[ia], h.a[iA], h.d[ia], h.d[iA]);
  if ((iA == ic || iB == ic) && a <= c && c <= b) {
    LS_TRY(hz_eval(eval, h, c, &pc, &dc));
    ic = (int)h.a.size() - 1;
    if (hz_wolfe(h, c, pc, dc)) { *iswolfe = true; *oA = *oB = ic; return 0; }
    int jA, jB;
    LS_TRY(hz_update(eval, h, iA, iB, ic, &jA, &jB));
    iA = jA; iB = jB;
  }
  *oA = iA; *oB = iB;
  return 0;
}
template <class Eval> int ls_hagerzhang(Eval &&eval, double phi_0, double dphi_0, double *alpha_out, bool *failed) {
  const double rho = 5.0, eps_hz = 1e-6, gamma = 0.66, psi3 = 0.1, feps = 2.220446049250313e-16;
  const int lsmax = 50;
  double alphamax = INFINITY;
  *failed = false;
  if (!(isfinite(phi_0) && isfinite(dphi_0)) || dphi_0 >= feps * fabs(phi_0)) { *alpha_out = 0.0; *failed = true; return 0; }
  hz_state h;
  h.a.push_back(0.0); h.v.push_back(phi_0); h.d.push_back(dphi_0);
  h.phi_0 = phi_0; h.dphi_0 = dphi_0;
  h.phi_lim = phi_0 + eps_hz * fabs(phi_0);
  double c = 1.0, phi_c, dphi_c;
  LS_TRY(eval(c, &phi_c, &dphi_c));
  for (int itf = 1; !(isfinite(phi_c) && isfinite(dphi_c)) && itf < 53; ++itf) {
    c *= psi3;
    LS_TRY(eval(c, &phi_c, &dphi_c));
  }
  if (!(isfinite(phi_c) && isfinite(dphi_c))) { *alpha_out = 0.0; return 0; }
  h.a.push_back(c); h.v.push_back(phi_c); h.d.push_back(dphi_c);
  bool bracketed = false;
  int ia = 0, ib = 1, it = 1;
  while (!bracketed && it < lsmax) {  // B0–B3
    if (dphi_c >= 0.0) {
      ib = (int)h.a.size() - 1;
      for (int i = ib - 1; i >= 0; --i)
        if (h.v[i] <= h.phi_lim) { ia = i; break; }
      bracketed = true;
    } else if (h.v.back() > h.phi_lim) {
      ib = (int)h.a.size() - 1;
      ia = 0;
      LS_TRY(hz_bisect(eval, h, &ia, &ib));
      bracketed = true;
    } else {
      const double cold = c;
      if (nextafter(cold, INFINITY) >= alphamax) { *alpha_out = cold; return 0; }
      c = fmin(c * rho, alphamax);
      LS_TRY(eval(c, &phi_c, &dphi_c));
      for (int itf = 1; !(isfinite(phi_c) && isfinite(dphi_c)) && c > nextafter(cold, INFINITY) && itf < 53; ++itf) {
        alphamax = c;
        c = (cold + c) / 2.0;
        LS_TRY(eval(c, &phi_c, &dphi_c));
      }
      if (!(isfinite(phi_c) && isfinite(dphi_c))) { *alpha_out = cold; return 0; }
      if (dphi_c < 0.0 && c == alphamax) { *alpha_out = c; return 0; }
      h.a.push_back(c); h.v.push_back(phi_c); h.d.push_back(dphi_c);
    }
    ++it;
  }
  while (it < lsmax) {  // L1–L3
    const double a = h.a[ia], b = h.a[ib];
    if (b - a <= nextafter(b, INFINITY) - b) { *alpha_out = a; return 0; }
    bool isw;
    int iA, iB;
    LS_TRY(hz_secant2(eval, h, ia, ib, &isw, &iA, &iB));
    if (h.lost) { *alpha_out = h.a[ia]; *failed = true; return 0; }
    if (isw) { *alpha_out = h.a[iA]; return 0; }
    const double A = h.a[iA], B = h.a[iB];
    if (B - A < gamma * (b - a)) {
      if (nextafter(h.v[ia], INFINITY) >= h.v[ib] && nextafter(h.v[iA], INFINITY) >= h.v[iB]) { *alpha_out = A; return 0; }
      ia = iA; ib = iB;
    } else {
      double pc, dc;
      LS_TRY(hz_eval(eval, h, (A + B) / 2.0, &pc, &dc));
      int ja, jb;
      LS_TRY(hz_update(eval, h, iA, iB, (int)h.a.size() - 1, &ja, &jb));
      ia = ja; ib = jb;
    }
    ++it;
  }
  *alpha_out = h.a[ia];  // iteration limit: LineSearchException in LineSearches.jl
  *failed = true;
  return 0;
}

// method: nk_options.linesearch, 2 = Static, 3 = StrongWolfe, 4 = MoreThuente, 5 = HagerZhang
template <class Eval> int ls_lsjl(Eval &&eval, int method, double *alpha_out, bool *failed) {
  *failed = false;
  double phi0, dphi0;
  LS_TRY(eval(0.0, &phi0, &dphi0));
  if (dphi0 >= 0.0) {  // not a descent direction: the full step, reported as a failed line search
    *alpha_out = 1.0;
    *failed = true;
    return 0;
  }
  switch (method) {
    case 2: return ls_static(eval, alpha_out);
    case 3: return ls_strongwolfe(eval, phi0, dphi0, alpha_out);
    case 4: return ls_morethuente(eval, phi0, dphi0, alpha_out);
    case 5: return ls_hagerzhang(eval, phi0, dphi0, alpha_out, failed);
    default: return LS_BAD_METHOD;
  }
}

#undef LS_TRY
