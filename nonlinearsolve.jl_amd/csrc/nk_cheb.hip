// The Chebyshev iteration on the device (declared in nk_internal.h): one first-step kernel, one unfused later-step kernel and
// the host driver that the polynomial preconditioner (nk_gmres.hip) and the multigrid smoothers (nk_mg.hip, nk_amg.hip) call.
// The library is built with -ffp-contract=off: the expressions below give the same bits wherever they are instantiated.
#include "nk_internal.h"
#include "nk_cheb.h"

#include <string.h>

#include <utility>
#include <vector>

// d = [dinv·]src/θ ; x = zero ? d : x + d ; r_copy = src (optional: the recurrence then continues on a private copy of b)
template <bool DINV>
__global__ __launch_bounds__(NK_BLOCK) void k_cheb_first(int64_t n, const double *__restrict__ src, const double *__restrict__ dinv,
                                                         double inv_theta, int zero, double *__restrict__ d, double *__restrict__ x,
                                                         double *__restrict__ r_copy, const int *d_skip) {
  if (nk_skip(d_skip)) return;
  const int64_t stride = (int64_t)gridDim.x * NK_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * NK_BLOCK + threadIdx.x; i < n; i += stride) {
    const double rv = src[i];
    double dd;
    if constexpr (DINV) dd = dinv[i] * rv * inv_theta;
    else dd = rv * inv_theta;
    if (r_copy) r_copy[i] = rv;
    d[i] = dd;
    x[i] = zero ? dd : x[i] + dd;
  }
}
// r −= A d (t holds A d) ; d = c1 d + c2 r ; x += d      (56 n bytes; every operand 16-byte aligned: checked by the driver)
__global__ __launch_bounds__(NK_BLOCK) void k_cheb_step(int64_t n, const double *__restrict__ t, double c1, double c2,
                                                        double *__restrict__ r, double *__restrict__ d, double *__restrict__ x,
                                                        const int *d_skip) {
  if (nk_skip(d_skip)) return;
  const int64_t npair = n >> 1, stride = (int64_t)gridDim.x * NK_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * NK_BLOCK + threadIdx.x; i < npair; i += stride) {
    const double2 tt = reinterpret_cast<const double2 *>(t)[i];
    double2 rr = reinterpret_cast<double2 *>(r)[i], dd = reinterpret_cast<double2 *>(d)[i],
            xx = reinterpret_cast<double2 *>(x)[i];
    rr.x -= tt.x; rr.y -= tt.y;
    dd.x = c1 * dd.x + c2 * rr.x; dd.y = c1 * dd.y + c2 * rr.y;
    xx.x += dd.x; xx.y += dd.y;
    reinterpret_cast<double2 *>(r)[i] = rr;
    reinterpret_cast<double2 *>(d)[i] = dd;
    reinterpret_cast<double2 *>(x)[i] = xx;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t i = n - 1;
    r[i] -= t[i];
    d[i] = c1 * d[i] + c2 * r[i];
    x[i] += d[i];
  }
}

int nk_cheb_run(nk_ctx *ctx, const nk_cheb_job &job, const nk_cheb_op &op, double **d_last) {
  const int64_t n = job.n;
  NK_REQUIRE(job.steps >= 1 && job.d && job.x && (job.zero ? job.b != nullptr : job.r != nullptr), "internal: Chebyshev job");
  NK_REQUIRE(job.steps == 1 || (job.r && job.t), "internal: Chebyshev steps beyond the first need r and t");
  NK_REQUIRE(job.fused || !job.dinv, "internal: the unfused Chebyshev step has no D⁻¹");
  nk_cheb_coef co(job.lmin, job.lmax);
  {
    const double *src = job.zero ? job.b : job.r;
    double *r_copy = job.zero ? job.r : nullptr;
    const dim3 grid(nk_grid_for(n, NK_BLOCK, 65536));
    if (job.dinv)
      NK_LAUNCH(ctx, k_cheb_first<true>, grid, dim3(NK_BLOCK), n, src, job.dinv, co.inv_theta(), job.zero ? 1 : 0, job.d, job.x,
                r_copy, job.d_skip);
    else
      NK_LAUNCH(ctx, k_cheb_first<false>, grid, dim3(NK_BLOCK), n, src, job.dinv, co.inv_theta(), job.zero ? 1 : 0, job.d, job.x,
                r_copy, job.d_skip);
  }
  double *dcur = job.d, *dnext = job.t;
  if (job.steps > 1 && !job.fused)
    NK_REQUIRE(((uintptr_t)job.t | (uintptr_t)job.r | (uintptr_t)job.d | (uintptr_t)job.x) % 16 == 0,
               "internal: the Chebyshev step's vectors must be 16-byte aligned");
  for (int k = 1; k < job.steps; ++k) {
    double c1, c2;
    co.next(&c1, &c2);
    if (job.fused) {   // d ping-pongs: the row epilogue writes d' while other rows still gather the old d
      nk_spmv_epi ep;
      ep.mode = NK_EPI_CHEB_STEP;
      ep.c1 = c1;
      ep.c2 = c2;
      ep.r = job.r;
      ep.dnew = dnext;
      ep.yacc = job.x;
      ep.dinv = job.dinv;
      NK_TRY(op(dcur, dnext, &ep));
      std::swap(dcur, dnext);
    } else {
      NK_TRY(op(job.d, job.t, nullptr));
      nk_prof_scope prof_(ctx, NK_K_OTHER, 56.0 * (double)n);
      NK_LAUNCH(ctx, k_cheb_step, dim3(nk_grid_for(n >> 1, NK_BLOCK, 4096)), dim3(NK_BLOCK), n, (const double *)job.t, c1, c2,
                job.r, job.d, job.x, job.d_skip);
    }
  }
  NK_HIP(hipGetLastError());
  if (d_last) *d_last = dcur;
  return NK_OK;
}

// ----------------------------------------------------------------------------- development harness (not in the public header)
// Test hook of tests/test_gpu_cheb.py, exported like nk_spmv_epilogue_test: nk_cheb_run on a CSR matrix, `fused` through the
// SpMV's row epilogue or not. HOST arrays of nrows doubles: b (read when `zero`) and dinv (nullable) in; x, r, d, t in and out;
// *last_in_t: whether the last correction ended in t. On the device every vector sits between guard words, checked afterwards.
extern "C" int nk_cheb_test(nk_csr *A, int steps, int zero, int fused, double lmin, double lmax, const double *b, const double *dinv,
                            double *x, double *r, double *d, double *t, int *last_in_t) {
  NK_REQUIRE(A && x && r && d && t && last_in_t && (b || !zero), "NULL argument");
  nk_ctx *ctx = A->ctx;
  NK_HIP(hipSetDevice(ctx->device));
  const size_t n = (size_t)A->nrows, G = 2;   // (two guard doubles: the vectors stay 16-byte aligned)
  const uint64_t canary = 0x7ff8c0de0000beefull;
  const double *in[6] = {b, dinv, x, r, d, t};
  std::vector<double *> dev(6, nullptr);
  auto guard = nk_make_guard(&dev, [](std::vector<double *> *p) { for (double *q : *p) hipFree(q); });
  std::vector<double> h(n + 2 * G);
  for (int i = 0; i < 6; ++i) {
    if (!in[i]) continue;
    for (size_t g = 0; g < G; ++g) { memcpy(&h[g], &canary, 8); memcpy(&h[G + n + g], &canary, 8); }
    if (n) memcpy(&h[G], in[i], n * sizeof(double));
    NK_TRY(nk_dev_alloc(&dev[i], h.size()));
    NK_HIP(nk_memcpy(ctx, dev[i], h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  auto at = [&](int i) { return dev[i] ? dev[i] + G : nullptr; };
  nk_cheb_job job;
  job.n = (int64_t)n;
  job.lmin = lmin;
  job.lmax = lmax;
  job.steps = steps;
  job.zero = zero != 0;
  job.fused = fused != 0;
  job.b = at(0);
  job.dinv = at(1);
  job.r = at(3);
  job.d = at(4);
  job.t = at(5);
  job.x = at(2);
  double *d_last = nullptr;
  NK_TRY(nk_cheb_run(ctx, job, [&](const double *dd, double *tt, const nk_spmv_epi *ep) {
    return nk_csr_spmv_dev(A, dd, ep ? nullptr : tt, nullptr, nullptr, ep);
  }, &d_last));
  NK_HIP(hipStreamSynchronize(ctx->stream));
  *last_in_t = d_last == job.t ? 1 : 0;
  double *out[6] = {nullptr, nullptr, x, r, d, t};
  for (int i = 0; i < 6; ++i) {
    if (!dev[i]) continue;
    NK_HIP(nk_memcpy(ctx, h.data(), dev[i], h.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t g = 0; g < G; ++g)
      NK_REQUIRE(memcmp(&h[g], &canary, 8) == 0 && memcmp(&h[G + n + g], &canary, 8) == 0, "guard word of vector %d overwritten", i);
    if (out[i] && n) memcpy(out[i], &h[G], n * sizeof(double));
  }
  return NK_OK;
}
