// What the compiled problem kinds — grids (nk_grid.hip), graphs (nk_graph.hip), elements (nk_elem.hip) — own and do alike: two
// loaded programs with three kernels, the parameter buffer, the pattern, the one launcher of a generated kernel, the problem
// object around them and the copies of their read-only data arrays. Plain functions over the plain struct nk_compiled
// (nk_internal.h) that every kind's state holds as a member. What a kind writes itself: its device types and kernels, its host
// tables, its contract, its validation and the argument list of its kernels.
#include "nk_internal.h"

int nk_compiled_load(nk_compiled_programs *C, const std::vector<char> &code_f, const std::vector<char> &code_j, const char *name_res,
                     const char *name_jvp, const char *name_jac, const char *what) {
  if (hipModuleLoadData(&C->mod_f, code_f.data()) != hipSuccess || hipModuleLoadData(&C->mod_jac, code_j.data()) != hipSuccess)
    NK_FAIL(NK_E_HIP, "hipModuleLoadData failed");
  if (hipModuleGetFunction(&C->fn_res, C->mod_f, name_res) != hipSuccess ||
      hipModuleGetFunction(&C->fn_jvp, C->mod_f, name_jvp) != hipSuccess ||
      hipModuleGetFunction(&C->fn_jac, C->mod_jac, name_jac) != hipSuccess)
    NK_FAIL(NK_E_HIP, "a generated %s kernel is missing from the compiled module", what);
  return NK_OK;
}

int nk_compiled_params_init(nk_compiled *C, const double *params, int nparams) {
  C->np = nparams;
  NK_TRY(nk_dev_alloc(&C->d_params, (size_t)(nparams > 0 ? nparams : 1)));
  if (nparams > 0 && params) NK_HIP(nk_memcpy(C->ctx, C->d_params, params, (size_t)nparams * sizeof(double), hipMemcpyHostToDevice));
  return NK_OK;
}

// Inside a profiled scope of the context (nk_problem_residual_dev, nk_problem_jvp_dev and nk_problem_jac_values_dev open one
// around the callback) the launch carries start / stop events like every NK_LAUNCH, so the generated kernels are timed by the
// same clock as the built-in ones.
int nk_compiled_launch(nk_compiled *C, hipFunction_t fn, int64_t items, void **args, void *stream) {
  const unsigned blocks = (unsigned)((items + 255) / 256);
  hipEvent_t e0, e1;
  hipError_t e;
  if (C->ctx->prof.on && (hipStream_t)stream == C->ctx->stream && nk_prof_next(C->ctx, &e0, &e1))
    e = hipExtModuleLaunchKernel(fn, blocks * 256u, 1, 1, 256, 1, 1, 0, (hipStream_t)stream, args, nullptr, e0, e1, 0);   // (sizes in threads)
  else
    e = hipModuleLaunchKernel(fn, blocks, 1, 1, 256, 1, 1, 0, (hipStream_t)stream, args, nullptr);   // (sizes in blocks)
  return e != hipSuccess;
}

void nk_compiled_unload(nk_compiled_programs *C) {
  if (C->mod_f) hipModuleUnload(C->mod_f);
  if (C->mod_jac) hipModuleUnload(C->mod_jac);
  C->mod_f = C->mod_jac = nullptr;
}

void nk_compiled_free(nk_compiled *C) {
  nk_compiled_unload(C);
  hipFree(C->d_params);
  nk_csr_destroy(C->pattern);
}

int nk_compiled_set_params(nk_problem *P, const double *params, int nparams) {
  nk_compiled *C = P->compiled;
  NK_REQUIRE(nparams == C->np, "nparams mismatch (%d vs %d)", nparams, C->np);
  NK_HIP(hipSetDevice(C->ctx->device));
  if (nparams > 0) NK_HIP(nk_memcpy(C->ctx, C->d_params, params, (size_t)nparams * sizeof(double), hipMemcpyHostToDevice));
  for (int i = 0; i < nparams && i < 8; ++i) P->params[i] = params[i];   // (the first eight, for inspection; the kernels read d_params)
  P->params_version++;
  nk_problem_invalidate(P);   // a Jacobian cached for the same u belongs to the old parameters
  return NK_OK;
}

int nk_compiled_problem(nk_compiled *C, int64_t n_local, int64_t n_global, int64_t row_begin, const double *params, int nparams,
                        const nk_user_callbacks &cb, void *user, nk_problem **out) {
  nk_problem *P = new nk_problem();
  P->ctx = C->ctx;
  P->kind = NK_PROBLEM_USER;
  P->n_local = n_local;
  P->n_global = n_global;
  P->row_begin = row_begin;
  P->nparams = nparams;
  for (int i = 0; params && i < nparams && i < 8; ++i) P->params[i] = params[i];
  P->cb = cb;   // (no vjp: Jᵀv is user_lin_J + the transposed SpMV)
  P->user = user;
  P->user_pattern = C->pattern;
  P->compiled = C;
  *out = P;
  return NK_OK;
}

// A NULL user pointer is refused exactly when there is something to copy. Only a graph without edges has an array of no
// elements: a grid has at least one node and a mesh at least one element and one node, so for them NULL is always refused.
int nk_compiled_data_copy(nk_problem *P, double *device_ptr, size_t bytes, const void *user_ptr, int memspace, bool to_device) {
  NK_REQUIRE(user_ptr || bytes == 0, "%s", to_device ? "NULL data" : "NULL out");
  NK_REQUIRE(memspace == NK_HOST || memspace == NK_DEVICE, "memspace = %d is neither NK_HOST nor NK_DEVICE", memspace);
  nk_ctx *ctx = P->compiled->ctx;
  NK_HIP(hipSetDevice(ctx->device));
  if (bytes == 0) return NK_OK;
  if (to_device)
    NK_HIP(nk_memcpy(ctx, device_ptr, user_ptr, bytes, memspace == NK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  else   // (a getter's user_ptr is its output)
    NK_HIP(nk_memcpy(ctx, const_cast<void *>(user_ptr), device_ptr, bytes, memspace == NK_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
  return NK_OK;
}
void nk_compiled_data_changed(nk_problem *P) {
  P->params_version++;
  nk_problem_invalidate(P);
}
