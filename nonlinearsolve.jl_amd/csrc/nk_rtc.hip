// hiprtc through dlopen, and the device-side prelude every run-time compiled kernel set starts with: the working precision
// and the forward-mode dual numbers; the cache of compiled programs and the copy-out of a code object. Shared by the ensemble
// kernels (nk_batch.hip: the prelude, the base options and the copy-out; it does not cache) and the compiled grid, graph and
// element problems (nk_grid.hip, nk_graph.hip, nk_elem.hip).
#include <dlfcn.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "nk_internal.h"

// ----------------------------------------------------------------------------- device source (compiled by hiprtc)
const char *const nk_dual_prelude = R"NKSRC(
// ---- the working precision: -DNK_F32 builds every solver kernel in single precision (flags & NK_BATCH_FLOAT32)
#ifdef NK_F32
typedef float nk_real;
#else
typedef double nk_real;
#endif
#define NK_R(x) ((nk_real)(x))
// ---- forward-mode dual numbers with NK_CH partials (ForwardDiff.Dual analogue)
struct Dual {
  nk_real v;
  nk_real d[NK_CH];
  __device__ Dual() {}
  __device__ Dual(nk_real x) : v(x) {
#pragma unroll
    for (int k = 0; k < NK_CH; ++k) d[k] = NK_R(0);
  }
};
#define NK_DUAL_LOOP _Pragma("unroll") for (int k = 0; k < NK_CH; ++k)
__device__ inline Dual operator+(const Dual &a, const Dual &b) { Dual r; r.v = a.v + b.v; NK_DUAL_LOOP r.d[k] = a.d[k] + b.d[k]; return r; }
__device__ inline Dual operator-(const Dual &a, const Dual &b) { Dual r; r.v = a.v - b.v; NK_DUAL_LOOP r.d[k] = a.d[k] - b.d[k]; return r; }
__device__ inline Dual operator-(const Dual &a) { Dual r; r.v = -a.v; NK_DUAL_LOOP r.d[k] = -a.d[k]; return r; }
__device__ inline Dual operator*(const Dual &a, const Dual &b) { Dual r; r.v = a.v * b.v; NK_DUAL_LOOP r.d[k] = a.d[k] * b.v + a.v * b.d[k]; return r; }
__device__ inline Dual operator/(const Dual &a, const Dual &b) {
  Dual r; const nk_real ib = NK_R(1) / b.v; r.v = a.v * ib;
  NK_DUAL_LOOP r.d[k] = (a.d[k] - r.v * b.d[k]) * ib;
  return r;
}
// scalar operands are taken in nk_real, so that `0.05 * u[i]` stays in the working precision on the dual path
__device__ inline Dual operator+(const Dual &a, nk_real b) { Dual r = a; r.v += b; return r; }
__device__ inline Dual operator+(nk_real b, const Dual &a) { Dual r = a; r.v += b; return r; }
__device__ inline Dual operator-(const Dual &a, nk_real b) { Dual r = a; r.v -= b; return r; }
__device__ inline Dual operator-(nk_real b, const Dual &a) { Dual r = -a; r.v += b; return r; }
__device__ inline Dual operator*(const Dual &a, nk_real b) { Dual r; r.v = a.v * b; NK_DUAL_LOOP r.d[k] = a.d[k] * b; return r; }
__device__ inline Dual operator*(nk_real b, const Dual &a) { return a * b; }
__device__ inline Dual operator/(const Dual &a, nk_real b) { return a * (NK_R(1) / b); }
__device__ inline Dual operator/(nk_real b, const Dual &a) { return Dual(b) / a; }
__device__ inline Dual &operator+=(Dual &a, const Dual &b) { a = a + b; return a; }
__device__ inline Dual &operator-=(Dual &a, const Dual &b) { a = a - b; return a; }
__device__ inline Dual &operator*=(Dual &a, const Dual &b) { a = a * b; return a; }
__device__ inline Dual &operator/=(Dual &a, const Dual &b) { a = a / b; return a; }
__device__ inline bool operator<(const Dual &a, const Dual &b) { return a.v < b.v; }
__device__ inline bool operator>(const Dual &a, const Dual &b) { return a.v > b.v; }
__device__ inline bool operator<=(const Dual &a, const Dual &b) { return a.v <= b.v; }
__device__ inline bool operator>=(const Dual &a, const Dual &b) { return a.v >= b.v; }
__device__ inline Dual nk_chain(const Dual &a, nk_real fv, nk_real dfv) { Dual r; r.v = fv; NK_DUAL_LOOP r.d[k] = dfv * a.d[k]; return r; }
__device__ inline Dual sqrt(const Dual &a) { const nk_real s = sqrt(a.v); return nk_chain(a, s, NK_R(0.5) / s); }
__device__ inline Dual exp(const Dual &a) { const nk_real e = exp(a.v); return nk_chain(a, e, e); }
__device__ inline Dual log(const Dual &a) { return nk_chain(a, log(a.v), NK_R(1) / a.v); }
__device__ inline Dual sin(const Dual &a) { return nk_chain(a, sin(a.v), cos(a.v)); }
__device__ inline Dual cos(const Dual &a) { return nk_chain(a, cos(a.v), -sin(a.v)); }
__device__ inline Dual tan(const Dual &a) { const nk_real t = tan(a.v); return nk_chain(a, t, NK_R(1) + t * t); }
__device__ inline Dual tanh(const Dual &a) { const nk_real t = tanh(a.v); return nk_chain(a, t, NK_R(1) - t * t); }
__device__ inline Dual atan(const Dual &a) { return nk_chain(a, atan(a.v), NK_R(1) / (NK_R(1) + a.v * a.v)); }
__device__ inline Dual fabs(const Dual &a) { return nk_chain(a, fabs(a.v), a.v < NK_R(0) ? NK_R(-1) : NK_R(1)); }
__device__ inline Dual pow(const Dual &a, nk_real e) { const nk_real pw = pow(a.v, e - NK_R(1)); return nk_chain(a, pw * a.v, e * pw); }
__device__ inline Dual pow(const Dual &a, int e) { return pow(a, (nk_real)e); }
#ifdef NK_F32
__device__ inline Dual pow(const Dual &a, double e) { return pow(a, (nk_real)e); }  // (else pow(u, 2.0) is ambiguous)
#endif
__device__ inline Dual pow(const Dual &a, const Dual &b) { return exp(b * log(a)); }
)NKSRC";

// after the prelude in the graph and element programs (-DNK_SEED_SET: 0 in the residual and JVP program, 1 in the fill's)
const char *const nk_seed_lift = R"NKSRC(
// an nk_real read from u becomes the source's T: itself, the dual with its one partial from v (NK_SEED_SET == 0), or the dual
// with the unit seed of component c if the value belongs to what the thread seeds (`hot`) and no partial otherwise
template <typename T> struct nk_lift;
template <> struct nk_lift<nk_real> {
  static __device__ __forceinline__ nk_real at(nk_real x, const nk_real *, int, int, bool) { return x; }
};
template <> struct nk_lift<Dual> {
  static __device__ __forceinline__ Dual at(nk_real x, const nk_real *__restrict__ v, int el, int c, bool hot) {
    Dual r;
    r.v = x;
#if NK_SEED_SET == 0
    r.d[0] = v[el];
#else
#pragma unroll
    for (int t = 0; t < NK_CH; ++t) r.d[t] = (hot && t == c) ? NK_R(1) : NK_R(0);
#endif
    return r;
  }
};
)NKSRC";

// ----------------------------------------------------------------------------- hiprtc through dlopen
typedef void *rtc_program;
static struct {
  void *h = nullptr;
  int (*Create)(rtc_program *, const char *, const char *, int, const char **, const char **) = nullptr;
  int (*Compile)(rtc_program, int, const char **) = nullptr;
  int (*LogSize)(rtc_program, size_t *) = nullptr;
  int (*Log)(rtc_program, char *) = nullptr;
  int (*CodeSize)(rtc_program, size_t *) = nullptr;
  int (*Code)(rtc_program, char *) = nullptr;
  int (*Destroy)(rtc_program *) = nullptr;
} RTC;

static int rtc_load() {
  if (RTC.h) return NK_OK;
  const char *names[] = {"libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"};
  for (const char *nm : names) {
    RTC.h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
    if (RTC.h) break;
  }
  if (!RTC.h) NK_FAIL(NK_E_UNSUPPORTED, "cannot dlopen libhiprtc (needed to compile the residual): %s", dlerror());
#define RTC_SYM(field, name)                                                          \
  RTC.field = (decltype(RTC.field))dlsym(RTC.h, name);                                \
  if (!RTC.field) { RTC.h = nullptr; NK_FAIL(NK_E_UNSUPPORTED, "libhiprtc lacks symbol %s", name); }
  RTC_SYM(Create, "hiprtcCreateProgram");
  RTC_SYM(Compile, "hiprtcCompileProgram");
  RTC_SYM(LogSize, "hiprtcGetProgramLogSize");
  RTC_SYM(Log, "hiprtcGetProgramLog");
  RTC_SYM(CodeSize, "hiprtcGetCodeSize");
  RTC_SYM(Code, "hiprtcGetCode");
  RTC_SYM(Destroy, "hiprtcDestroyProgram");
#undef RTC_SYM
  return NK_OK;
}

// Compile `full` with `opts`: the code object into `code`, the compiler's log into `log`. *failed = the source did not
// compile (the caller words the message: it knows the contract the source was written against); any other trouble is an error.
int nk_rtc_compile(const std::string &full, const char *name, const std::vector<const char *> &opts, std::vector<char> *code,
                   std::string *log, bool *failed) {
  *failed = false;
  NK_TRY(rtc_load());
  rtc_program prog = nullptr;
  if (RTC.Create(&prog, full.c_str(), name, 0, nullptr, nullptr) != 0) NK_FAIL(NK_E_HIP, "hiprtcCreateProgram failed");
  const int rc = RTC.Compile(prog, (int)opts.size(), const_cast<const char **>(opts.data()));
  size_t ls = 0;
  RTC.LogSize(prog, &ls);
  if (ls > 1 && log) { log->resize(ls); RTC.Log(prog, &(*log)[0]); }
  if (rc != 0) {
    RTC.Destroy(&prog);
    *failed = true;
    return NK_OK;
  }
  size_t cs = 0;
  RTC.CodeSize(prog, &cs);
  code->resize(cs);
  RTC.Code(prog, code->data());
  RTC.Destroy(&prog);
  return NK_OK;
}

// ----------------------------------------------------------------------------- the programs of the compiled problems
std::vector<const char *> nk_rtc_base_options() { return {"--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17"}; }

// The same text with the same options gives the same code object: a problem created again (another size, another context) skips
// the compiler. One cache for all kinds; the key holds all that varies between two programs — the program's name (so that two
// kinds never share an entry), its options and `varying`, the part of `full` that is not the same for every program of the name.
// A source that does not compile is not cached.
int nk_rtc_program(const std::string &full, const char *name, const std::vector<std::string> &defs, const std::string &varying,
                   const char *what, const char *contract, std::vector<char> *code, std::string *log) {
  std::vector<const char *> opts = nk_rtc_base_options();
  for (const std::string &d : defs) opts.push_back(d.c_str());
  static std::mutex mtx;
  static std::map<std::string, std::vector<char>> cache;
  std::string key = std::string(name) + ' ';
  for (const char *o : opts) { key += o; key += ' '; }
  key += varying;
  {
    std::lock_guard<std::mutex> lock(mtx);
    auto it = cache.find(key);
    if (it != cache.end()) { *code = it->second; return NK_OK; }
  }
  bool failed = false;
  NK_TRY(nk_rtc_compile(full, name, opts, code, log, &failed));
  if (failed)
    NK_FAIL(NK_E_INVALID, "%s residual source does not compile (%s): %.900s", what, contract,
            log && !log->empty() ? log->c_str() : "(no log)");
  std::lock_guard<std::mutex> lock(mtx);
  cache[key] = *code;
  return NK_OK;
}

// a code object handed out for inspection: *bytes gets its size; buf may be NULL to ask for the size only
int nk_rtc_copy_out(const std::vector<char> &code, void *buf, int64_t capacity, int64_t *bytes) {
  *bytes = (int64_t)code.size();
  if (!buf) return NK_OK;
  NK_REQUIRE(capacity >= *bytes, "buffer of %lld bytes, the code object has %lld", (long long)capacity, (long long)*bytes);
  memcpy(buf, code.data(), code.size());
  return NK_OK;
}
