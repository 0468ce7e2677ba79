// lmm_api.hip -- host orchestration + C ABI (include/lmm_hip.h) of liblmm_hip.so.
//
// One process drives ONE MI355X (one process per GPU; the multi-GPU layer above shards latents and
// sums partial results with one RCCL all-reduce).  Latent problems are independent, so each latent of the
// shard gets a slot = (factor-matrix buffer, HIP stream); slots run concurrently so one latent's
// latency-bound 64x64 diagonal-block step overlaps the other latents' MFMA trailing updates.
//
// Blocked Cholesky: recursive halving on column ranges,
//     potrf(j0, w):  potrf(j0, h);  C[j0+h:, j0+h:j0+w] -= A[j0+h:, j0:j0+h] A[j0+h:j0+w, j0:j0+h]';  potrf(j0+h, w-h)
// so that >95 % of the n^3/3 flops run in large-K f64-MFMA updates that read/write each trailing tile once
// per level (log2(n/64) levels) instead of once per panel.  Leaves (64 columns): diag64 (factor + inverse
// of the diagonal block) then TRSM as a GEMM with the inverse.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "lmm_internal.h"
#include "lmm_emul.h"

namespace {

constexpr double kLog2Pi = 1.8378770664093453;
constexpr int kMaxStreams = 16;

struct Ctx {
  bool init = false;
  int device = -1;
  int nstreams = 4;
  hipStream_t streams[kMaxStreams];
  hipEvent_t ev_main;
  hipEvent_t ev_slot[kMaxStreams];
  // pinned host arena for the small per-call uploads / read-backs (projection matrices, per-latent results): copies from / to
  // pinned memory are truly asynchronous, pageable ones stall the calling thread until the stream has drained
  char* pin = nullptr;
  size_t pin_cap = 0, pin_off = 0;
  char* pin_dev = nullptr;           // the arena as the device addresses it (hipHostGetDevicePointer); nullptr: not mapped
  std::vector<void*> scratch;          // device blocks that live until the NEXT API call starts (call_scratch)
  struct EmulBlock { void* p; size_t bytes; };
  std::map<hipStream_t, EmulBlock> emul_blocks;   // scratch of the emulated updates: ONE block per stream per API call, shared by that stream's batches
  bool emul_denied = false;            // this API call could not get such a block: its remaining batches take the f64 path without asking again
  int* region_flags = nullptr;         // dependency flags of potrf_region_kernel: [stream][matrix][region_flag_ints], zeroed ONCE (lmm_init)
                                       // -- every launch tags its flags with a fresh epoch, so they never need resetting
  std::multimap<size_t, void*> pool;   // cached device blocks (size -> ptr)
  std::map<void*, size_t> live;
  std::string err;
  int err_latent = -1, err_info = 0;
  // multi-GPU: one RCCL communicator per process (rank = this GPU)
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_world = 0;
  hipEvent_t ev_caller = nullptr;
  // measurement hooks
  bool prof = false, prof_serial = false;
  struct ProfRec { int cls; double work, bytes; hipEvent_t e0, e1; int M, N, K, count; };
  std::vector<ProfRec> prof_recs;
  std::vector<hipEvent_t> ev_pool;
};
Ctx g;
std::mutex g_mu;
int g_proj = 0;   // lmm_proj_dtype of the H unprojection of predictive marginals (lmm_set_projection_dtype)

// H unprojection of latent marginals (reference src/oilmm.jl:69,72) in the selected projection dtype
void mix_marginals(const double* lat, int ns, int ml, const double* Hm, int p, int pw, double lat_add, double out_add, double* out,
                   hipStream_t st) {
  if (g_proj == LMM_PROJ_NATIVE || ml == 0) launch_mix(lat, ns, ml, Hm, p, pw, lat_add, out_add, nullptr, 0.0, out, st);
  else launch_mix_bf16(lat, ns, ml, Hm, p, pw, lat_add, out_add, g_proj == LMM_PROJ_BF16X2 ? 2 : 1, out, st);
}

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g.err = buf;
  return code;
}

#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) throw fail(LMM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                     __FILE__, __LINE__);                                         \
  } while (0)

// bytes from the pinned arena (valid until the next API call), or nullptr when it is full / absent
void* pin_take(size_t bytes) {
  bytes = (bytes + 63) & ~size_t(63);
  if (g.pin == nullptr || g.pin_off + bytes > g.pin_cap) return nullptr;
  void* p = g.pin + g.pin_off;
  g.pin_off += bytes;
  return p;
}

// device-side alias of a pointer into the pinned arena (kernels write small results straight into host memory: no copy back)
template <typename T>
T* pin_dev(T* host) {
  if (host == nullptr || g.pin_dev == nullptr) return nullptr;
  return reinterpret_cast<T*>(g.pin_dev + (reinterpret_cast<char*>(host) - g.pin));
}

void* dev_alloc(size_t bytes) {
  if (bytes == 0) bytes = 256;
  bytes = (bytes + 255) & ~size_t(255);
  auto it = g.pool.find(bytes);
  void* p = nullptr;
  if (it != g.pool.end()) {
    p = it->second;
    g.pool.erase(it);
  } else {
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {   // release the cache and retry once
      for (auto& kv : g.pool) (void)hipFree(kv.second);
      g.pool.clear();
      (void)hipGetLastError();
      e = hipMalloc(&p, bytes);
      if (e != hipSuccess) throw fail(LMM_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    }
  }
  g.live[p] = bytes;
  return p;
}

void dev_free(void* p) {
  if (!p) return;
  auto it = g.live.find(p);
  if (it == g.live.end()) return;
  g.pool.insert({it->second, p});
  g.live.erase(it);
}

// Scratch that kernels queued by this API call use: handed back to the pool when the NEXT call starts (every entry point returns
// with its streams drained, and error paths drain the device), so it is never recycled while in flight.
double* call_scratch(size_t count) {
  void* p = dev_alloc(count * sizeof(double));
  g.scratch.push_back(p);
  return static_cast<double*>(p);
}
void release_call_scratch() {
  for (void* p : g.scratch) dev_free(p);
  g.scratch.clear();
  g.emul_blocks.clear();
  g.emul_denied = false;
}
// call_scratch that may be refused: nullptr when neither the pool nor hipMalloc has a block of that size (the pool is NOT flushed
// and no error is recorded: the caller has another way)
void* call_scratch_try(size_t bytes) {
  bytes = (bytes + 255) & ~size_t(255);
  void* p = nullptr;
  auto it = g.pool.find(bytes);
  if (it != g.pool.end()) { p = it->second; g.pool.erase(it); }
  else if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  g.live[p] = bytes;
  g.scratch.push_back(p);
  return p;
}

template <typename T>
struct Buf {   // RAII device buffer from the caching pool
  T* p = nullptr;
  size_t n = 0;
  bool own = true;       // false: p is borrowed (a device alias into the pinned arena), not returned to the pool
  Buf() = default;
  explicit Buf(size_t count) : p(static_cast<T*>(dev_alloc(count * sizeof(T)))), n(count) {}
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p(o.p), n(o.n), own(o.own) { o.p = nullptr; o.n = 0; }
  Buf& operator=(Buf&& o) noexcept { if (this != &o) { if (own) dev_free(p); p = o.p; n = o.n; own = o.own; o.p = nullptr; o.n = 0; } return *this; }
  ~Buf() { if (own) dev_free(p); }
};

bool is_device_ptr(const void* p) {
  hipPointerAttribute_t a;
  hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// A read-only input that may live on host or device: gives a device pointer valid on stream st.
struct DevIn {
  const double* p = nullptr;
  Buf<double> own;
  DevIn(const double* src, size_t count, hipStream_t st) {
    if (src == nullptr) return;
    if (is_device_ptr(src)) { p = src; return; }
    own = Buf<double>(count);
    HIPCHK(hipMemcpyAsync(own.p, src, count * sizeof(double), hipMemcpyHostToDevice, st));
    p = own.p;
  }
};

// An output that may live on host or device.
struct DevOut {
  double* dst; double* p; size_t count; Buf<double> own; bool direct;
  DevOut(double* dst_, size_t count_) : dst(dst_), p(nullptr), count(count_), direct(false) {
    if (dst == nullptr) return;
    if (is_device_ptr(dst)) { p = dst; direct = true; }
    else { own = Buf<double>(count); p = own.p; }
  }
  void finish(hipStream_t st) {
    if (dst && !direct) HIPCHK(hipMemcpyAsync(dst, p, count * sizeof(double), hipMemcpyDeviceToHost, st));
  }
};

inline int rup(int v, int m) { return (v + m - 1) / m * m; }
// leading dimension for `rows` rows: keeps column starts off the same HBM channel / L2 set
inline int pad_ld(int rows) { return (rows % 512) == 0 ? rows + 16 : rows; }

// fp32 compute mode (lmm_set_compute_dtype): MATRICES (factor matrices, inverse diagonal blocks, cross-solve blocks) are float
// buffers; they are still carried as Buf<double> / double* (opaque to the host, which never dereferences them), sized by
// mat_count(elements) doubles.  Vectors stay double.
inline size_t mat_count(size_t elems) { return g_f32 ? (elems + 1) / 2 : elems; }
inline double mat_bytes(double elems) { return elems * (g_f32 ? 4.0 : 8.0); }
// element `off` of a matrix buffer in the current storage type, as the double* the launch wrappers take
inline double* mat_at(double* p, size_t off) { return g_f32 ? reinterpret_cast<double*>(reinterpret_cast<float*>(p) + off) : p + off; }

// ---- allocation-extent guard -------------------------------------------------------------------------------------------------
// Every launch below that reads or writes a rows x cols block (leading dimension ld) of a POOLED buffer is preceded by this check of
// the block against the allocation the pointer lies in: a mismatch between two roundings of the same size (round 3: cross-solve
// blocks kept rup(n*, 64) rows while the Schur complement read rup(n*, 128) of them -- an out-of-bounds device read at n* = 9 that a
// later run hid) becomes LMM_ERR_ARG before anything is launched, instead of a fault.  Pointers outside the pool (caller memory)
// are not checked.  matrix: the block is in the compute dtype (Float32 elements in the fp32 mode), else Float64.
void guard_extent(const void* p, size_t rows, size_t ld, size_t cols, bool matrix, const char* what) {
  if (p == nullptr || rows == 0 || cols == 0) return;
  auto it = g.live.upper_bound(const_cast<void*>(p));
  if (it == g.live.begin()) return;
  --it;
  const char* b0 = static_cast<const char*>(it->first);
  const char* b1 = b0 + it->second;
  const char* q = static_cast<const char*>(p);
  if (q >= b1) return;                                   // not inside a pooled block
  const size_t eb = (matrix && g_f32) ? 4 : 8;
  const size_t need = ((cols - 1) * ld + rows) * eb;
  if (rows > ld || q + need > b1)
    throw fail(LMM_ERR_ARG, "internal extent check failed: %s touches %zu x %zu (ld %zu) = %zu bytes at offset %zu of a %zu-byte allocation",
               what, rows, cols, ld, need, (size_t)(q - b0), it->second);
}
// (a launch covers the matrix rows [64 row_tile0, nrows), stored from buffer row 64 row_tile0 - row_shift on: buffer rows < nrows - row_shift)
void guard_gram(const GramArgs& a, const char* what) {
  if (64 * a.row_tile0 < a.row_shift) throw fail(LMM_ERR_ARG, "internal extent check failed: %s starts above its buffer (row tile %d, shift %d)", what, a.row_tile0, a.row_shift);
  guard_extent(a.A, (size_t)(a.nrows - a.row_shift), (size_t)a.ld, (size_t)a.ncols, true, what);
}
void gram_g(const GramArgs& a, hipStream_t st, const char* what = "Gram assembly") { guard_gram(a, what); launch_gram(a, st); }
void gram_batch_g(const GramArgs* ga, int nb, hipStream_t st, const char* what = "Gram assembly") {
  for (int j = 0; j < nb; ++j) guard_gram(ga[j], what);
  launch_gram_batch(ga, nb, st);
}
// C (M x N, ldc) -= A (M x K, lda) B (N x K, ldb)'
void gemm_nt_g(double* C, int ldc, const double* A, int lda, const double* B, int ldb, int M, int N, int K, int lower, bool set,
               hipStream_t st, const char* what) {
  guard_extent(C, M, ldc, N, true, what); guard_extent(A, M, lda, K, true, what); guard_extent(B, N, ldb, K, true, what);
  launch_gemm_nt(C, ldc, A, lda, B, ldb, M, N, K, lower, set, st);
}
void gemm_nt_g(const BatchPtr& C, size_t offC, int ldc, const BatchPtr& A, size_t offA, int lda, const BatchPtr& B, size_t offB, int ldb,
               int M, int N, int K, int lower, bool set, int nb, hipStream_t st, const char* what, bool no_splitk = false) {
  const size_t eb = g_f32 ? 4 : 8;
  for (int j = 0; j < nb; ++j) {
    guard_extent(reinterpret_cast<const char*>(C.p[j]) + offC * eb, M, ldc, N, true, what);
    guard_extent(reinterpret_cast<const char*>(A.p[j]) + offA * eb, M, lda, K, true, what);
    guard_extent(reinterpret_cast<const char*>(B.p[j]) + offB * eb, N, ldb, K, true, what);
  }
  launch_gemm_nt(C, offC, ldc, A, offA, lda, B, offB, ldb, M, N, K, lower, set, nb, st, no_splitk);
}
void rider_stats_g(const double* R, int ld, int nr, int nk, const double* z, double mu, double base, double* partial,
                   double* mean_out, double* var_out, hipStream_t st) {
  if (R) guard_extent(R, nr, ld, nk, true, "rider statistics (R)");
  launch_rider_stats(R, ld, nr, nk, z, mu, base, partial, mean_out, var_out, st);
}

// Brackets one launch with events when profiling is on (lmm_profile_begin); otherwise just launches.
struct ProfScope {
  bool on; hipStream_t st; size_t idx;
  ProfScope(int cls, double work, hipStream_t st_, int M = 0, int N = 0, int K = 0, double bytes = 0.0, int count = 1)
      : on(g.prof), st(st_), idx(0) {      // count: launches bracketed by this one event pair
    if (!on) return;
    Ctx::ProfRec r; r.cls = cls; r.work = work; r.bytes = bytes; r.M = M; r.N = N; r.K = K; r.count = count;
    for (hipEvent_t* e : {&r.e0, &r.e1}) {
      if (!g.ev_pool.empty()) { *e = g.ev_pool.back(); g.ev_pool.pop_back(); }
      else HIPCHK(hipEventCreate(e));
    }
    HIPCHK(hipEventRecord(r.e0, st));
    idx = g.prof_recs.size();
    g.prof_recs.push_back(r);
  }
  ~ProfScope() { if (on) (void)hipEventRecord(g.prof_recs[idx].e1, st); }
};

inline int eff_streams() { return (g.prof && g.prof_serial) ? 1 : g.nstreams; }

struct Dims {
  int n, NC, NR, ld;
  Dims(int n_, int nrider) : n(n_) {
    NC = rup(std::max(n, 1), 128);      // whole 128-column panels (round 3: the panel / region kernels work on them; the pad is identity)
    NR = rup(NC + std::max(nrider, 0), 64);
    ld = pad_ld(NR);
  }
  size_t elems() const { return (size_t)ld * NC; }
};

// ---- latent kernels, resolved ------------------------------------------------------------------------------------------------
// The user-facing registry (lmm_ard_create / lmm_kernel_tag_create / lmm_kernel_sum_create / _destroy / _grad) maps a tag to d
// per-dimension factors, an RQ shape alpha, or the terms of a sum kernel, and keeps the tag's latest gradient; it has its own mutex
// and never takes the context lock for longer than a try-lock on an error message.  A caller's lmm_gp_t names a tag in the high bits
// of `kind`.  An entry point turns its caller's array into a LatentSet ONCE (resolve, under the context lock) and everything below
// it takes `const Latent&`: a caller's descriptor and a resolved latent are different types.
//   KernelTerm  one base kernel V kappa_kind(|x - x'| ./ l).  With factors, l_k = mult * ard[k]: all-equal factors (or d == 1) fold
//               into the isotropic lengthscale mult * fold; other factors are uploaded as 1 / l_k.  `ev` evaluates the term; `gd` is
//               what the gradient reduction takes (d > 1 with factors, folded or not: the per-dimension reduction with
//               inv_ls = 1 / mult; else `ev`).
//   Latent      the caller's mean, variance and lengthscale and nt >= 1 terms.  A plain latent is its one term (v_c = l_c = 1,
//               V = variance); a sum latent (kind LMM_KERNEL_SUM) has the terms of its sum tag, V_c = variance v_c and
//               mult_c = lengthscale l_c, and their `ev` on the device (dterms).  "One term" is a host-side view: a plain latent
//               keeps its base kind on the device and is never evaluated as a sum.
//   LatentSet   the latents of one call and the host / device buffers their descriptors point into.  Terms with equal (tag, mult)
//               share one uploaded vector, so equal plain latents compare equal (Latent::same_kernel).  Held by shared_ptr by the
//               running call and by every posterior handle built from it (own copy of the factors: tags may go).
#define LMM_ARD_MAX_TAGS 4096
struct ArdTag {           // d = 0: no factors; alpha = 0: no shape; terms non-empty: a sum tag (lmm_kernel_sum_create; d = 0, alpha = 0)
  int d; std::vector<double> ard, grad; double alpha = 0.0, galpha = 0.0;
  double rho = 0.0, grho = 0.0;         // a periodic latent's rho (lmm_kernel_tag_create_periodic; 0: none) and its latest gradient
  double decay = 0.0, gdecay = 0.0;     // a locally periodic latent's decay (lmm_kernel_tag_create_locally_periodic, with its rho; 0: none)
  double quality = 0.0, gquality = 0.0; // an SHO latent's quality factor (lmm_kernel_tag_create_sho; 0: none) and its latest gradient
  std::vector<lmm_gp_t> terms;
  std::vector<lmm_gp_grad_t> tgrad;     // a sum tag's latest per-term (d/dv_c, d/dl_c, 0)
  bool statespace = false;              // a sum tag of lmm_kernel_sum_create_statespace: its terms may be SHO; the state-space entry points alone take it
};
std::mutex g_ard_mu;
std::map<int, ArdTag> g_ard_tags;
int g_ard_next = 1;

#define LMM_RQ_DEFAULT_ALPHA 2.0          // KernelFunctions' RationalQuadraticKernel(; alpha = 2.0)

struct KernelTerm {
  int tag = 0;                     // the user tag its factors and alpha come from (0: none)
  bool has_ard = false;            // the tag has factors
  double mult = 1.0, fold = 1.0;   // multiplier of the factors; the factor a folded term's lengthscale was multiplied by (1 otherwise)
  double alpha = 0.0;              // the tag's RQ shape (0: none; the term then reports no alpha gradient)
  double rho = 0.0;                // the tag's periodic rho (0: none: rho = 1, and the term reports no rho gradient)
  double quality = 0.0;            // the tag's SHO quality (0: none: Q = 1, and the term reports no quality gradient)
  double decay = 0.0;              // the tag's locally periodic decay (0: none: decay = 1, and the term reports no decay gradient)
  double dscale = 1.0;             // what multiplies the decay: a sum latent's s0 (the outer ScaleTransform acts on the SE factor too), else 1
  double v = 1.0, ls = 1.0;        // v_c, l_c
  LatentDev ev{}, gd{};
  int ev_ent = -1, gd_ent = -1;    // entries of LatentSet::host that ev.ils / gd.ils point to (-1: isotropic)
};

struct Latent {
  double variance = 1.0, lengthscale = 1.0, mean = 0.0;   // lengthscale: a folded plain latent's includes the fold factor
  int kind = 0, tag = 0;                                  // base kind or LMM_KERNEL_SUM; user tag (0: none)
  double quality = 1.0;                                   // an SHO latent's quality factor (its tag's, 1 without one)
  std::vector<KernelTerm> terms;
  const LatentDev* dterms = nullptr;                      // a sum latent's terms[c].ev on the device
  bool is_sum() const { return kind == LMM_KERNEL_SUM; }
  int nt() const { return (int)terms.size(); }
  bool has_periodic() const {
    for (const KernelTerm& T : terms) if (T.ev.kind == LMM_KERNEL_PERIODIC || T.ev.kind == LMM_KERNEL_LOCALLY_PERIODIC) return true;
    return false;
  }
  LatentDev dev() const {
    if (!is_sum()) { LatentDev d = terms[0].ev; d.mean = mean; return d; }
    LatentDev d{};
    d.kind = kind; d.var = variance; d.inv_ls = 1.0 / lengthscale; d.mean = mean; d.alpha = LMM_RQ_DEFAULT_ALPHA;
    d.terms = dterms; d.nterms = nt();
    return d;
  }
  // kernel fields of a Gram assembly
  void set_kernel(GramArgs& a) const {
    const LatentDev d = dev();
    a.kind = d.kind; a.var = d.var; a.inv_ls = d.inv_ls; a.ils = d.ils; a.alpha = d.alpha; a.terms = d.terms; a.nterms = d.nterms;
    a.sum_per = is_sum() && has_periodic();
    a.inv_decay = d.inv_decay;
  }
  // kappa(0): the variance, or v0 sum_c v_c for a sum latent
  double prior_var() const {
    if (!is_sum()) return variance;
    double v = 0.0;
    for (const KernelTerm& T : terms) v += T.ev.var;
    return v;
  }
  // The descriptor in the dense-H latent array (DenseArgs.lat, the posterior's latd): the dense kernels read var as kappa(0).
  LatentDev dense_dev() const { LatentDev d = dev(); d.var = prior_var(); return d; }
  // Whether two latents have the same kernel (the dense-H decoupled shortcut).  A sum latent's term with per-dimension lengthscales
  // counts as different.
  bool same_kernel(const Latent& o) const {
    if (kind != o.kind || variance != o.variance || lengthscale != o.lengthscale || nt() != o.nt()) return false;
    for (int c = 0; c < nt(); ++c) {
      const LatentDev& x = terms[c].ev;
      const LatentDev& y = o.terms[c].ev;
      if (x.kind != y.kind || x.var != y.var || x.inv_ls != y.inv_ls || x.alpha != y.alpha || x.inv_decay != y.inv_decay) return false;
      if (is_sum() ? (x.ils != nullptr || y.ils != nullptr) : x.ils != y.ils) return false;
    }
    return true;
  }
};

// The sum mode of the latents [l0, l1), which names the instantiation of the dense-H and inducing-point kernels that serves them
// (mode_dispatch): 2 with a (locally) periodic latent or term, 1 with a sum latent, else 0.
static int sum_mode(const Latent* lts, int l0, int l1) {
  int mode = 0;
  for (int l = l0; l < l1; ++l) {
    if (lts[l].has_periodic()) return 2;
    if (lts[l].is_sum()) mode = 1;
  }
  return mode;
}

struct LatentSet {
  int d = 0;
  std::vector<Latent> lat;
  std::vector<double> host;                 // effective inverse lengthscales, d per entry
  Buf<double> dev;                          // the same on the device
  std::vector<LatentDev> thost;             // the evaluation descriptors of every sum term (host, then `tdev`)
  Buf<LatentDev> tdev;
  int any_sum() const { return sum_mode(lat.data(), 0, (int)lat.size()); }      // the dense kernels' instantiation
  // d of the per-dimension gradient reduction (0: every term takes the isotropic one)
  int ard_grad_d() const {
    for (const Latent& L : lat)
      for (const KernelTerm& T : L.terms) if (T.gd.ils) return d;
    return 0;
  }
  // Gradient entry points: the per-dimension reduction keeps d sums in registers (LMM_ARD_GRAD_DMAX).
  int ard_grad_check() const {
    if (d <= LMM_ARD_GRAD_DMAX || !ard_grad_d()) return LMM_OK;
    return fail(LMM_ERR_UNSUPPORTED, "gradients of ARD latents are served for d <= %d (d = %d)", LMM_ARD_GRAD_DMAX, d);
  }
  // first[k] = index of the first term of latent l0 + k among the terms of the latents [l0, l1); first[l1 - l0] = their number
  std::vector<int> term_offsets(int l0, int l1) const {
    std::vector<int> first(l1 - l0 + 1, 0);
    for (int l = l0; l < l1; ++l) first[l - l0 + 1] = first[l - l0] + lat[l].nt();
    return first;
  }
};

// One term from its base kind, V, multiplier E and the factors / shape of its tag: fold, d == 1, or a (shared) vector.  A periodic
// term's descriptor carries 1 / rho^2 in the alpha slot, which it does not otherwise use (so same_kernel compares rho with it); a
// locally periodic one the same and 1 / (dscale decay) in inv_decay (the factors and E act on its period only).
void resolve_term(LatentSet& S, KernelTerm& T, int base, double V, double E, const std::vector<double>& ard, double alpha, double rho,
                  double decay, double dscale, std::map<std::pair<int, double>, int>& entry_of) {
  const int d = S.d;
  T.mult = E; T.alpha = alpha; T.rho = rho; T.decay = decay; T.dscale = dscale;
  LatentDev ev{};
  ev.kind = base; ev.var = V; ev.inv_ls = 1.0 / E; ev.alpha = alpha > 0.0 ? alpha : LMM_RQ_DEFAULT_ALPHA;
  if (base == LMM_KERNEL_PERIODIC || base == LMM_KERNEL_LOCALLY_PERIODIC) ev.alpha = rho > 0.0 ? 1.0 / (rho * rho) : 1.0;
  if (base == LMM_KERNEL_LOCALLY_PERIODIC) ev.inv_decay = 1.0 / (dscale * (decay > 0.0 ? decay : 1.0));
  T.gd = ev;
  if (!ard.empty()) {
    T.has_ard = true;
    bool equal = true;
    for (int k = 1; k < d; ++k) equal = equal && ard[k] == ard[0];
    if (equal) { T.fold = ard[0]; ev.inv_ls = 1.0 / (E * ard[0]); }      // exactly the isotropic term of lengthscale E * ard[0]
    if (d > 1) {                           // the gradient reduction needs the per-dimension vector, folded or not
      auto key = std::make_pair(T.tag, E);
      auto it = entry_of.find(key);
      if (it == entry_of.end()) {
        it = entry_of.emplace(key, (int)(S.host.size() / d)).first;
        for (int k = 0; k < d; ++k) S.host.push_back(1.0 / (E * ard[k]));
      }
      T.gd_ent = it->second;
      if (!equal) T.ev_ent = it->second;
    } else T.gd = ev;                      // d == 1: the isotropic reduction at l_eff = E * ard[0] gives the one derivative
  }
  T.ev = ev;
}

// A latent without a tag (no validation: resolve has done it)
Latent plain_latent(const lmm_gp_t& gp) {
  Latent L;
  L.variance = gp.variance; L.lengthscale = gp.lengthscale; L.mean = gp.mean; L.kind = gp.kind & LMM_KERNEL_BASE_MASK;
  L.terms.resize(1);
  LatentDev& ev = L.terms[0].ev;
  ev.kind = L.kind; ev.var = gp.variance; ev.inv_ls = 1.0 / gp.lengthscale; ev.alpha = LMM_RQ_DEFAULT_ALPHA;
  if (L.kind == LMM_KERNEL_PERIODIC || L.kind == LMM_KERNEL_LOCALLY_PERIODIC) ev.alpha = 1.0;      // 1 / rho^2 at the default rho = 1
  if (L.kind == LMM_KERNEL_LOCALLY_PERIODIC) ev.inv_decay = 1.0;                                   // and the default decay = 1
  if (L.kind == LMM_KERNEL_SHO) ev.alpha = 1.0;                                                    // an SHO latent's quality (Q = 1 without a tag)
  L.terms[0].mult = gp.lengthscale;
  L.terms[0].gd = ev;
  return L;
}

// Whether a tag's shape (alpha: RQ; rho alone: periodic; rho and decay: locally periodic; none: any kind) fits a base kind.
inline bool tag_shape_fits(int base, double alpha, double rho, double decay) {
  if (alpha > 0.0 && base != LMM_KERNEL_RQ) return false;
  if (decay > 0.0) return base == LMM_KERNEL_LOCALLY_PERIODIC;
  if (rho > 0.0 && base != LMM_KERNEL_PERIODIC) return false;
  return true;
}
inline bool base_kind_ok(int base) { return base <= LMM_KERNEL_RQ || base == LMM_KERNEL_PERIODIC || base == LMM_KERNEL_LOCALLY_PERIODIC; }

// The caller's latents, validated and resolved.  A call without tags allocates nothing on the device and copies nothing to it.
// An SHO latent (LMM_KERNEL_SHO) is served over a one-dimensional input only: d > 1 is refused here, before any device work.  Its
// descriptor carries the quality in the alpha slot (as RQ its shape).  The entry points that do not serve it (input gradients, the
// inducing-point bound) refuse it right after this (refuse_sho), so no route evaluates another kernel in its place.
// statespace: the caller is a state-space entry point, which alone takes a sum tag of lmm_kernel_sum_create_statespace (its terms may be
// SHO, with their quality tags); everywhere else such a latent is refused by name here, before any device work.
int resolve(const lmm_gp_t* gps, int m, int d, std::shared_ptr<LatentSet>& out, bool statespace = false) {
  if (!gps) return fail(LMM_ERR_ARG, "gps is NULL");
  for (int l = 0; l < m; ++l) {
    const int base = gps[l].kind & LMM_KERNEL_BASE_MASK;
    if (gps[l].kind >= 0 && base == LMM_KERNEL_SHO) {
      if (d != 1) {
        g.err_latent = l; g.err_info = 0;
        return fail(LMM_ERR_UNSUPPORTED, "latent %d: an SHO latent (kernel kind %d) is served over a one-dimensional input only (d = %d)", l, LMM_KERNEL_SHO, d);
      }
      if (!(gps[l].variance > 0.0) || !(gps[l].lengthscale > 0.0)) return fail(LMM_ERR_ARG, "latent %d: variance and lengthscale must be > 0", l);
      continue;
    }
    if (gps[l].kind < 0 || (base != LMM_KERNEL_SUM && !base_kind_ok(base))) return fail(LMM_ERR_UNSUPPORTED, "latent %d: unsupported kernel kind %d", l, gps[l].kind);
    if (base == LMM_KERNEL_SUM && (gps[l].kind >> 8) == 0) return fail(LMM_ERR_ARG, "latent %d: a sum latent needs a sum tag (lmm_kernel_sum_create)", l);
    if (!(gps[l].variance > 0.0) || !(gps[l].lengthscale > 0.0)) return fail(LMM_ERR_ARG, "latent %d: variance and lengthscale must be > 0", l);
  }
  auto S = std::make_shared<LatentSet>();
  S->d = d;
  S->lat.resize(m);
  std::map<std::pair<int, double>, int> entry_of;     // (tag, multiplier) -> entry of S->host
  for (int l = 0; l < m; ++l) {
    Latent& L = S->lat[l];
    L = plain_latent(gps[l]);
    const int tag = gps[l].kind >> 8;
    if (tag == 0) continue;
    L.tag = tag;
    std::vector<double> ard;
    double alpha, rho, decay, quality;
    std::vector<lmm_gp_t> terms;
    std::vector<std::vector<double>> tard;
    std::vector<double> talpha, trho, tdecay, tquality;
    {
      std::lock_guard<std::mutex> lk(g_ard_mu);
      auto it = g_ard_tags.find(tag);
      if (it == g_ard_tags.end()) return fail(LMM_ERR_ARG, "latent %d: unknown or destroyed ARD tag %d", l, tag);
      if (L.is_sum() != !it->second.terms.empty())
        return fail(LMM_ERR_ARG, "latent %d: tag %d is %sa sum tag but the kernel kind is %d", l, tag, L.is_sum() ? "not " : "", L.kind);
      if (it->second.d != 0 && it->second.d != d)
        return fail(LMM_ERR_DIM, "latent %d: ARD tag %d has %d dimensions, the inputs have %d", l, tag, it->second.d, d);
      if (it->second.statespace && !statespace) {
        g.err_latent = l; g.err_info = 0;
        return fail(LMM_ERR_UNSUPPORTED, "latent %d: sum tag %d comes from lmm_kernel_sum_create_statespace, which the state-space entry points alone serve", l, tag);
      }
      ard = it->second.ard;
      alpha = it->second.alpha;
      rho = it->second.rho;
      decay = it->second.decay;
      quality = it->second.quality;
      terms = it->second.terms;
      for (size_t c = 0; c < terms.size(); ++c) {
        const int tt = terms[c].kind >> 8;
        tard.emplace_back();
        talpha.push_back(0.0);
        trho.push_back(0.0);
        tdecay.push_back(0.0);
        tquality.push_back(0.0);
        if (tt == 0) continue;
        auto jt = g_ard_tags.find(tt);
        if (jt == g_ard_tags.end() || !jt->second.terms.empty())
          return fail(LMM_ERR_ARG, "latent %d: term %d: unknown or destroyed tag %d", l, (int)c, tt);
        if (jt->second.d != 0 && jt->second.d != d)
          return fail(LMM_ERR_DIM, "latent %d: term %d: tag %d has %d dimensions, the inputs have %d", l, (int)c, tt, jt->second.d, d);
        tard.back() = jt->second.ard;
        talpha.back() = jt->second.alpha;
        trho.back() = jt->second.rho;
        tdecay.back() = jt->second.decay;
        tquality.back() = jt->second.quality;
        const int tb = terms[c].kind & LMM_KERNEL_BASE_MASK;
        if (!tag_shape_fits(tb, talpha.back(), trho.back(), tdecay.back()) || (jt->second.quality > 0.0) != (tb == LMM_KERNEL_SHO))
          return fail(LMM_ERR_ARG, "latent %d: term %d: tag %d carries a shape its kernel kind %d does not take", l, (int)c, tt, tb);
      }
    }
    if (quality > 0.0 && L.kind != LMM_KERNEL_SHO)
      return fail(LMM_ERR_ARG, "latent %d: tag %d carries an SHO quality but the kernel kind is %d", l, tag, L.kind);
    if (L.kind == LMM_KERNEL_SHO) {
      if (!(quality > 0.0))
        return fail(LMM_ERR_ARG, "latent %d: tag %d carries %s but the kernel kind is %d, which takes a quality only", l, tag,
                    !ard.empty() ? "factors" : alpha > 0.0 ? "an RQ shape" : decay > 0.0 ? "a locally periodic rho and decay" : "a periodic rho", L.kind);
      L.quality = quality;
      KernelTerm& T = L.terms[0];
      T.tag = tag; T.quality = quality; T.ev.alpha = quality; T.gd = T.ev;
      continue;
    }
    if (L.is_sum()) {
      L.terms.assign(terms.size(), KernelTerm{});
      for (int c = 0; c < L.nt(); ++c) {
        KernelTerm& T = L.terms[c];
        T.tag = terms[c].kind >> 8; T.v = terms[c].variance; T.ls = terms[c].lengthscale;
        resolve_term(*S, T, terms[c].kind & LMM_KERNEL_BASE_MASK, L.variance * T.v, L.lengthscale * T.ls, tard[c], talpha[c], trho[c], tdecay[c],
                     L.lengthscale, entry_of);
        if (T.ev.kind == LMM_KERNEL_SHO) {      // an SHO term (a state-space sum tag): its quality in the alpha slot, as an SHO latent's (Q = 1 without a tag)
          T.quality = tquality[c];
          T.ev.alpha = T.quality > 0.0 ? T.quality : 1.0;
          T.gd = T.ev;
        }
      }
      continue;
    }
    if (alpha > 0.0 && L.kind != LMM_KERNEL_RQ)
      return fail(LMM_ERR_ARG, "latent %d: tag %d carries an RQ shape but the kernel kind is %d", l, tag, L.kind);
    if (!tag_shape_fits(L.kind, alpha, rho, decay))
      return fail(LMM_ERR_ARG, "latent %d: tag %d carries a %s but the kernel kind is %d", l, tag,
                  decay > 0.0 ? "locally periodic rho and decay" : "periodic rho", L.kind);
    KernelTerm& T = L.terms[0];
    T.tag = tag;
    resolve_term(*S, T, L.kind, L.variance, L.lengthscale, ard, alpha, rho, decay, 1.0, entry_of);
    L.lengthscale = gps[l].lengthscale * T.fold;
  }
  if (!S->host.empty()) {
    S->dev = Buf<double>(S->host.size());
    // (S->host lives as long as the set, so the copy may complete asynchronously; every launch that reads it is ordered behind st0)
    HIPCHK(hipMemcpyAsync(S->dev.p, S->host.data(), S->host.size() * sizeof(double), hipMemcpyHostToDevice, g.streams[0]));
    for (Latent& L : S->lat)
      for (KernelTerm& T : L.terms) {
        if (T.ev_ent >= 0) T.ev.ils = S->dev.p + (size_t)T.ev_ent * d;
        if (T.gd_ent >= 0) T.gd.ils = S->dev.p + (size_t)T.gd_ent * d;
      }
  }
  // the sum latents' evaluation descriptors on the device
  for (const Latent& L : S->lat)
    if (L.is_sum()) for (const KernelTerm& T : L.terms) S->thost.push_back(T.ev);
  if (!S->thost.empty()) {
    S->tdev = Buf<LatentDev>(S->thost.size());
    HIPCHK(hipMemcpyAsync(S->tdev.p, S->thost.data(), S->thost.size() * sizeof(LatentDev), hipMemcpyHostToDevice, g.streams[0]));
    size_t off = 0;
    for (Latent& L : S->lat)
      if (L.is_sum()) { L.dterms = S->tdev.p + off; off += L.nt(); }
  }
  out = std::move(S);
  return LMM_OK;
}
// The entry points' preamble: `lts` is the resolved array every internal function takes.
#define RESOLVE(gps, m, d)                                  \
  std::shared_ptr<LatentSet> ls;                            \
  if (int rc_ = resolve(gps, m, d, ls)) return rc_;         \
  const Latent* lts = ls->lat.data()
inline int shard_check(int l0, int l1, int m) {
  return (l0 < 0 || l1 > m || l0 > l1) ? fail(LMM_ERR_ARG, "bad latent shard") : (int)LMM_OK;
}
inline std::vector<double> latent_means(const Latent* lts, int m) {
  std::vector<double> means(m);
  for (int l = 0; l < m; ++l) means[l] = lts[l].mean;
  return means;
}

// The preamble of the per-latent entry points that take training data (x, y, [U, S, sigma2,] gps, shard), in three pieces in the order
// the error codes are pinned in; train() is all three, and an entry point with checks of its own between two pieces calls the pieces.
//   train_args     `bad` (the entry point's own NULL / size test), m > p, then with TRAIN_SIGMA2 / TRAIN_S the noise and S checks, the shard
//   train_resolve  the latents resolved, the shard's bounds and the host means
//   Train::upload  x and y on the device
// An entry point that checks sigma2 elsewhere in its order (after its latents are resolved) does so itself, after train().
enum { TRAIN_SIGMA2 = 1, TRAIN_S = 2 };
struct Shard {
  std::shared_ptr<LatentSet> ls;
  const Latent* lts = nullptr;         // all m latents
  int l0 = 0, l1 = 0, ms = 0, mk = 1;  // the shard, its latents, max(ms, 1)
  void set(int l0_, int l1_) { lts = ls->lat.data(); l0 = l0_; l1 = l1_; ms = l1 - l0; mk = std::max(ms, 1); }
};
struct Train : Shard {
  std::vector<double> means;           // of all m latents
  DevIn xd{nullptr, 0, nullptr}, yd{nullptr, 0, nullptr};
  void upload(const double* x, size_t nx, const double* y, size_t ny) {
    xd = DevIn(x, nx, g.streams[0]); yd = DevIn(y, ny, g.streams[0]);
  }
};
int train_args(bool bad, int p, int m, const double* S, double sigma2, int l0, int l1, int checks) {
  if (bad) return fail(LMM_ERR_ARG, "bad arguments");
  if (m > p) return fail(LMM_ERR_DIM, "out dim of x != out dim of f.");
  if ((checks & TRAIN_SIGMA2) && !(sigma2 > 0.0)) return fail(LMM_ERR_ARG, "sigma2 must be > 0");
  if (checks & TRAIN_S)
    for (int l = 0; l < m; ++l)
      if (!(S[l] > 0.0) || !std::isfinite(S[l])) return fail(LMM_ERR_ARG, "S must be finite and > 0 (S[%d] = %g)", l, S[l]);
  return shard_check(l0, l1, m);
}
int train_resolve(const lmm_gp_t* gps, int m, int d, int l0, int l1, Train& T) {
  if (int rc = resolve(gps, m, d, T.ls)) return rc;
  T.set(l0, l1);
  T.means = latent_means(T.lts, m);
  return LMM_OK;
}
// x: d x n; y: ny values (n p, or n p ncol).  p = m and S = nullptr for an IndependentMOGP.
int train(bool bad, const double* x, int d, int n, const double* y, size_t ny, int p, const double* S, int m, double sigma2,
          const lmm_gp_t* gps, int l0, int l1, int checks, Train& T) {
  if (int rc = train_args(bad, p, m, S, sigma2, l0, l1, checks)) return rc;
  if (int rc = train_resolve(gps, m, d, l0, l1, T)) return rc;
  T.upload(x, (size_t)d * n, y, ny);
  return LMM_OK;
}

// An entry point that does not serve SHO latents names the first one (what: the entry point's service, for the message).
int refuse_sho(const LatentSet& S, const char* what) {
  for (size_t l = 0; l < S.lat.size(); ++l)
    if (S.lat[l].kind == LMM_KERNEL_SHO) {
      g.err_latent = (int)l; g.err_info = 0;
      return fail(LMM_ERR_UNSUPPORTED, "latent %d: %s not served for an SHO latent (kernel kind %d)", (int)l, what, LMM_KERNEL_SHO);
    }
  return LMM_OK;
}

// Posterior latent mean mu + K(xs, x) alpha (launch_post_mean): one pass per term, added in term order.
void post_mean_g(const double* xs, int ns, const double* x, int n, int d, const double* alpha, const Latent& L, double* partial,
                 double* out, hipStream_t st) {
  if (alpha == nullptr || n == 0) { launch_post_mean(xs, ns, x, n, d, alpha, L.dev(), partial, out, st); return; }
  double* tmp = L.nt() > 1 ? call_scratch(ns) : nullptr;
  for (int c = 0; c < L.nt(); ++c) {
    LatentDev tc = L.terms[c].ev;
    tc.mean = c == 0 ? L.mean : 0.0;
    launch_post_mean(xs, ns, x, n, d, alpha, tc, partial, c == 0 ? out : tmp, st);
    if (c > 0) launch_vec_lin(out, tmp, 1.0, ns, out, st);
  }
}

// The input gradient (grad_x_kernel) keeps d sums per row in registers, as the ARD reduction does.
int input_grad_check(int d, bool wanted) {
  if (!wanted || d <= LMM_ARD_GRAD_DMAX) return LMM_OK;
  return fail(LMM_ERR_UNSUPPORTED, "gradients with respect to the inputs are served for d <= %d (d = %d)", LMM_ARD_GRAD_DMAX, d);
}

// Chain rule of a latent from its term reductions: term c's kernel is V_c kappa_c(. / E_c) with V_c = v0 v_c and E_c = s0 l_c, so
// d/dv_c = v0 d/dV_c, d/dl_c = s0 d/dE_c and d/ds0 = sum_c l_c d/dE_c (returned; a plain latent's d/d lengthscale).  red: LMM_NGRAD
// sums per term, ard: d per-dimension sums per term (read where gd.ils is set).  aa, tr: alpha.alpha and tr Kt^-1 over all rows
// (d/dV_c = (sum_{i>j} w K_c,ij + V_c (aa - tr) / 2) / V_c; *dv0 = sum_c v_c d/dV_c).  out: one record of term_grad_stride(d) values
// per term: (d/dv_c, d/dl_c, d/dalpha_c or d/drho_c, d/ddecay_c, d/dl_k of the term's per-dimension lengthscales).  A locally periodic
// term's SE lengthscale is dscale * decay (dscale = s0 in a sum): red[9] is the derivative with respect to that product, so
// d/ddecay_c = dscale red[9] and, in a sum, d/ds0 gains decay red[9].
inline size_t term_grad_stride(int d) { return 4 + (size_t)d; }
double grad_finish(const Latent& L, int d, const double* red, const double* ard, double aa, double tr, double* out,
                   double* dv0 = nullptr) {
  double ds0 = 0.0, gv0 = 0.0;
  const size_t sw = term_grad_stride(d);
  for (int c = 0; c < L.nt(); ++c) {
    const KernelTerm& T = L.terms[c];
    const double* rc = red + (size_t)LMM_NGRAD * c;
    double* o = out + sw * c;
    const double V = T.ev.var;
    const double gV = (rc[7] + 0.5 * V * (aa - tr)) / V;
    const double dE = T.gd.ils ? rc[0] : rc[0] * T.fold;
    o[0] = gV * L.variance;
    o[1] = dE * L.lengthscale;
    o[2] = (T.alpha > 0.0 || T.rho > 0.0 || T.quality > 0.0) ? rc[8] : 0.0;      // d/d alpha (RQ), d/d rho (periodic) or d/d quality (SHO): one slot, a term has one of them
    if (T.gd.ils) for (int k = 0; k < d; ++k) o[4 + k] = ard[(size_t)d * c + k];
    else if (T.has_ard) o[4] = rc[0];                      // d == 1: d/d l_eff, l_eff = multiplier * fold
    ds0 += dE * T.ls;
    if (T.ev.kind == LMM_KERNEL_LOCALLY_PERIODIC) {
      o[3] = T.decay > 0.0 ? T.dscale * rc[9] : 0.0;
      if (L.is_sum()) ds0 += (T.decay > 0.0 ? T.decay : 1.0) * rc[9];
    }
    gv0 += gV * T.v;
  }
  if (dv0) *dv0 = gv0;
  return ds0;
}
// Publishes a gradient call's records (trec: m x LMM_SUM_MAX_TERMS of them, grad_finish) to the registry: every tag the call named is
// reset; then, over the latents [l0, l1), a sum tag gets (d/dv_c, d/dl_c, 0) per term and each term's tag d/d ard[k] = multiplier *
// d/d l_k and, with an RQ shape, d/d alpha (with a periodic rho, d/d rho), summed over the terms carrying it.  trec == nullptr (grad_gps NULL): zeros.
void publish_grads(const LatentSet& S, const std::vector<double>* trec, int l0, int l1) {
  bool any = false;
  for (const Latent& L : S.lat) any = any || L.tag != 0;
  if (!any) return;
  std::lock_guard<std::mutex> lk(g_ard_mu);
  auto reset = [&](int tag) {
    auto it = g_ard_tags.find(tag);
    if (tag == 0 || it == g_ard_tags.end()) return;
    it->second.grad.assign(it->second.d, 0.0); it->second.galpha = 0.0; it->second.grho = 0.0; it->second.gdecay = 0.0; it->second.gquality = 0.0;
    it->second.tgrad.assign(it->second.terms.size(), lmm_gp_grad_t{0.0, 0.0, 0.0});
  };
  for (const Latent& L : S.lat) {
    reset(L.tag);
    for (const KernelTerm& T : L.terms) reset(T.tag);
  }
  if (!trec) return;
  const size_t sw = term_grad_stride(S.d);
  for (int l = l0; l < l1; ++l) {
    const Latent& L = S.lat[l];
    auto st = L.is_sum() ? g_ard_tags.find(L.tag) : g_ard_tags.end();
    for (int c = 0; c < L.nt(); ++c) {
      const KernelTerm& T = L.terms[c];
      const double* r = &(*trec)[((size_t)l * LMM_SUM_MAX_TERMS + c) * sw];
      if (st != g_ard_tags.end() && (size_t)c < st->second.tgrad.size()) {
        st->second.tgrad[c].variance += r[0]; st->second.tgrad[c].lengthscale += r[1];
      }
      auto it = g_ard_tags.find(T.tag);
      if (T.tag == 0 || it == g_ard_tags.end()) continue;
      if (T.has_ard)
        for (int k = 0; k < std::min(S.d, it->second.d); ++k) it->second.grad[k] += T.mult * r[4 + k];
      if (T.alpha > 0.0) it->second.galpha += r[2];
      if (T.rho > 0.0) it->second.grho += r[2];
      if (T.quality > 0.0) it->second.gquality += r[2];
      if (T.decay > 0.0) it->second.gdecay += r[3];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// blocked factorisation drivers
// ------------------------------------------------------------------------------------------------
inline int split(int w) { return potrf_split(w); }      // left width of the recursive split (lmm_potrf_plan.h)

// A batch of up to LMM_MAX_BATCH same-shaped factor matrices factored in lock-step by the same launches
// (blockIdx.y / blockIdx.x selects the matrix): the small recursion levels then fill the chip and the launch
// count per latent drops by the batch size.
struct Batch {
  int nb = 0;
  BatchPtr A{}, W{};
  BatchInfo info{};
  void add(double* a, double* w, int* i) { A.p[nb] = a; W.p[nb] = w; info.p[nb] = i; ++nb; }
};

static int g_in_flight = 1;       // batches that run concurrently on the slot streams (fork_slots / join_slots)
// lmm_dev_f64_screen_stats: with g_f64_screen_stats on, every factorisation ends by copying its screened steps' counters here (M, N, K, dead tiles, ran)
static int g_f64_screen_stats = 0;
static std::vector<int> g_f64_screen_last;
// lmm_dev_zero_extent_stats: likewise, the void work items of every step that takes the zero extents (kind, j0, h, N, M, count, shape word)
static int g_zero_ext_stats = 0;
static std::vector<int> g_zero_ext_last;
inline int sw_region_cols() { return factor_switches().region; }      // widest block column of one region launch (LMM_REGION; 0: off)
// `bytes` of call scratch, a multiple of 8 as scratch_round makes them (lmm_potrf_plan.h); nullptr for none
template <class T> T* scratch_bytes(size_t bytes) { return bytes ? reinterpret_cast<T*>(call_scratch(bytes / 8)) : nullptr; }
// The zero extents of a batch (lmm_emul.h): [matrix][zero_ext_ld(NR)] ints in call scratch, set to LMM_ZERO_EXT_NONE on the stream; the
// Gram launch that assembles the batch lowers them (GramArgs.zext).  nullptr when the switch is off or the matrices are not Float64.
int* zero_ext_scratch(int NR, int nb, hipStream_t st) {
  if (g_f32 || !factor_switches().zero_extents) return nullptr;
  const size_t ints = (size_t)zero_ext_ld(NR) * nb;
  int* p = scratch_bytes<int>(scratch_ints(ints));
  guard_extent(p, scratch_ints(ints) / 8, scratch_ints(ints) / 8, 1, false, "zero extents");
  HIPCHK(hipMemsetAsync(p, 0x7F, ints * sizeof(int), st));
  return p;
}
static PotrfPlan emul_view(int NR, int NC, int nb) { return plan_potrf_emul_view(NR, NC, nb, factor_switches()); }
// The test hooks' read-back of a per-step counter array (n ints; nullptr: the factorisation kept none): copied to the host, which
// synchronises the stream, and handed to fmt step by step, which appends what the hook reports to `last`.
template <class F>
void read_step_counters(const int* dev, size_t n, const PotrfPlan& P, hipStream_t st, std::vector<int>& last, F fmt) {
  last.clear();
  if (dev == nullptr) return;
  std::vector<int> h(n);
  HIPCHK(hipMemcpyAsync(h.data(), dev, n * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (size_t i = 0; i < P.steps.size(); ++i) fmt(P.steps[i], i, h, last);
}

// Entry point of the factorisation of a batch: columns [0, NC) of every matrix (rows 0 .. NR - 1 participate; W: NC / 64 inverse
// diagonal blocks).  plan_potrf decides what is launched, which scratch it needs and how the steps are wired to it; this function
// checks the plan once, takes the scratch it lists -- all of it lives until the API call ends -- and launches the steps.
// zext (may be nullptr: nothing is left out): the batch's zero extents, matrix j's at zext + j * zero_ext_ld(NR) -- valid only if the
// launch that wrote them is the only writer of the factor matrices so far.
void potrf_batch(const Batch& B, int ld, int NR, int NC, int n_real, hipStream_t st, int rows_real = -1, const int* zext = nullptr) {
  for (int j = 0; j < B.nb; ++j) {
    guard_extent(B.A.p[j], NR, ld, NC, true, "factorisation (factor matrix)");
    guard_extent(B.W.p[j], 64, 64, (size_t)(NC / 64) * 64, true, "factorisation (inverse diagonal blocks)");
  }
  auto make_plan = [&]() {
    return plan_potrf(NR, NC, B.nb, rows_real, g_in_flight, device_cus(), g_f32 != 0, (ld & 1) != 0, g_strict_progress != 0, !g.emul_denied, factor_switches(),
                      zext != nullptr, g_zero_ext_stats != 0);
  };
  PotrfPlan P = make_plan();
  // Scratch of the emulated updates: ONE block per stream per API call (g.emul_blocks): the batches a stream factors one after the
  // other share it (stream order keeps them apart), so an API call holds at most one block per stream it uses however many batches it
  // has -- plus the smaller ones a stream outgrew, if its batches differ in shape.  If a block cannot be had the f64 path runs, for the
  // rest of the call (said once per process on stderr).
  void* emul_blk = nullptr;
  if (P.emul_bytes > 0) {
    auto it = g.emul_blocks.find(st);
    emul_blk = (it != g.emul_blocks.end() && it->second.bytes >= P.emul_bytes) ? it->second.p : nullptr;
    if (emul_blk == nullptr) {
      emul_blk = call_scratch_try(P.emul_bytes);
      if (emul_blk != nullptr) g.emul_blocks[st] = Ctx::EmulBlock{emul_blk, P.emul_bytes};
      else {
        g.emul_denied = true;
        static bool said = false;
        if (!said) { said = true; fprintf(stderr, "lmm: no %zu-byte scratch for the int8-emulated updates: they run on the f64 kernel\n", P.emul_bytes); }
        P = make_plan();
      }
    }
  }
  if (const PotrfViolation v = plan_potrf_check(P, NR)) {
    const PotrfStep& s = P.steps[v.step];
    throw fail(LMM_ERR_ARG, "internal extent check failed: step %d (kind %d, %d x %d x %d at column %d of %d rows): %s: %lld against %lld", v.step, s.kind, s.M, s.N,
               s.h, s.j0, NR, potrf_invariant_text(v.which), v.needs, v.has);
  }
  if (!P.zext) zext = nullptr;
  guard_extent(zext, P.zext_bytes / 8, P.zext_bytes / 8, 1, false, "factorisation (zero extents)");
  const size_t nsteps = P.steps.size();
  auto per_matrix = [&](size_t doubles) {
    BatchPtr S{};
    double* base = call_scratch(doubles * B.nb);
    for (int j = 0; j < B.nb; ++j) S.p[j] = base + doubles * j;
    return S;
  };
  BatchPtr W2{}, asst{};
  BatchInfo flags{};
  if (P.w2_doubles) W2 = per_matrix(P.w2_doubles);
  if (P.region_cols > 0) {                 // dependency flags of the region launches: this stream's slice of the persistent, once-zeroed
    int si = -1;                           // array (launches are told apart by epoch); an unknown stream gets a zeroed scratch
    for (int s = 0; s < kMaxStreams; ++s) if (g.streams[s] == st) si = s;
    const size_t fi = region_flag_ints(NR);
    int* fl;
    if (si >= 0 && g.region_flags) fl = g.region_flags + (size_t)si * LMM_MAX_BATCH * fi;
    else {
      fl = scratch_bytes<int>(scratch_ints(fi * B.nb));
      HIPCHK(hipMemsetAsync(fl, 0, fi * sizeof(int) * B.nb, st));
    }
    for (int j = 0; j < B.nb; ++j) flags.p[j] = fl + fi * j;
  }
  int* nflags = scratch_bytes<int>(scratch_ints(P.node_flag_ints * B.nb));
  if (nflags) HIPCHK(hipMemsetAsync(nflags, 0, P.node_flag_ints * B.nb * sizeof(int), st));
  if (P.asst_doubles) asst = per_matrix(P.asst_doubles);
  std::vector<unsigned long long*> amax_kept(nsteps, nullptr);
  for (size_t i = 0; i < nsteps; ++i)
    if (P.steps[i].keeps_amax) amax_kept[i] = scratch_bytes<unsigned long long>(P.amax_bytes);
  unsigned char* scr_flags = scratch_bytes<unsigned char>(P.f64_flag_bytes);
  int* scr_stat = scratch_bytes<int>(P.f64_stat_bytes);
  if (scr_stat) HIPCHK(hipMemsetAsync(scr_stat, 0, nsteps * 2 * sizeof(int), st));
  void* emul_aux_blk = scratch_bytes<void>(P.emul_aux_bytes);
  void* emul_screen_blk = scratch_bytes<void>(P.emul_screen_bytes);
  unsigned long long* emul_bmax = scratch_bytes<unsigned long long>(P.emul_bmax_bytes);
  int* zx_stat = scratch_bytes<int>(P.zext_stat_bytes);
  if (zx_stat) HIPCHK(hipMemsetAsync(zx_stat, 0, nsteps * sizeof(int), st));
  std::vector<int> region_n128(nsteps, 0);
  auto zx_of = [&](int si) { ZeroExt z; z.p = zext; z.ld = zero_ext_ld(NR); z.stat = zx_stat ? zx_stat + si : nullptr; return z; };
  // the step's kept array, and the earlier steps' arrays its cover reads
  auto keep_of = [&](int si, unsigned long long* bmax, int ncb) {
    const PotrfStep& s = P.steps[si];
    EmulAmaxKeep keep{amax_kept[si], NR, s.j0 + s.h, s.cover.n, {}, s.cover.scan0 - s.j0, bmax, s.j0 / 128, ncb};
    for (int q = 0; q < s.cover.n; ++q) keep.src[q] = amax_kept[s.cover.step[q]];
    return keep;
  };
  auto leaf128 = [&](int c) { launch_leaf128(B.A, (size_t)c * ld + c, ld, B.W, (size_t)(c / 64) * 4096, W2, (size_t)(c / 128) * 16384, c, n_real, B.info, B.nb, st); };
  for (int si = 0; si < (int)nsteps; ++si) {
    const PotrfStep& s = P.steps[si];
    const bool named = s.named();
    ProfScope ps(s.cls, s.work, st, named ? s.M : 0, named ? s.N : 0, named ? s.h : 0, s.bytes);
    const int j0 = s.j0, r0 = s.j0 + s.h;
    const size_t offW = (size_t)(j0 / 64) * 4096, offA = (size_t)j0 * ld + r0;      // the inverse block at j0; the rows from r0 of the columns from j0
    switch (s.kind) {
      case POTRF_DIAG64: launch_diag64(B.A, (size_t)j0 * ld + j0, ld, B.W, offW, j0, n_real, B.info, B.nb, st); break;
      case POTRF_SOLVE64: launch_gemm_nt(B.A, offA, ld, B.A, offA, ld, B.W, offW, 64, s.M, 64, 64, 0, true, B.nb, st); break;
      case POTRF_UPDATE: launch_gemm_nt(B.A, (size_t)r0 * ld + r0, ld, B.A, offA, ld, B.A, offA, ld, s.M, s.N, s.h, 1, false, B.nb, st); break;
      case POTRF_LEAF128: leaf128(j0); break;
      case POTRF_PANEL_BULK: launch_panel_bulk(B.A, W2, ld, NR, j0, B.nb, st); break;
      case POTRF_UPDATE_LEAF:
        if (s.screened) {
          guard_extent(scr_flags, s.flag_bytes / 8, s.flag_bytes / 8, 1, false, "screened update (tile flags)");
          guard_extent(scr_stat, nsteps, nsteps, 1, false, "screened update (counters)");
          HIPCHK(launch_f64_screen(B.A, (size_t)r0 * ld + r0, ld, B.A, offA, ld, s.M, s.N, s.h, s.strip, B.nb, keep_of(si, nullptr, 0), scr_flags, scr_stat + 2 * si,
                                   s.vote_from >= 0 ? scr_stat + 2 * s.vote_from : nullptr, st, zx_of(si), r0));
        }
        launch_update_leaf(B.A, B.W, W2, B.info, ld, NR, j0, s.h, s.N, n_real, B.nb, st, s.strip, s.fused_bulk ? nflags : nullptr, (int)P.node_flag_ints,
                           s.screened ? scr_flags : nullptr, zx_of(si));
        break;
      case POTRF_EMUL_UPDATE_LEAF: {
        guard_extent(emul_blk, s.scratch / 8, s.scratch / 8, 1, false, "emulated update (scratch)");
        guard_extent(emul_screen_blk, s.screen_bytes / 8, s.screen_bytes / 8, 1, false, "emulated update (screen)");
        const EmulAmaxKeep keep = keep_of(si, emul_bmax, P.emul_ncb);
        HIPCHK(launch_emul_update(B.A, (size_t)r0 * ld + r0, ld, B.A, offA, ld, s.M, s.N, s.h, B.nb, s.group, P.emul_nmod, emul_blk, emul_aux_blk, emul_screen_blk, st, &keep, zx_of(si), r0));
        leaf128(r0);
        break;
      }
      case POTRF_REGION: region_n128[si] = launch_region(B.A, B.W, W2, B.info, flags, ld, NR, j0, s.N, n_real, B.nb, s.first_done, st, rows_real, &asst, zx_of(si)); break;
    }
  }
  if (g_f64_screen_stats)        // test hook only
    read_step_counters(scr_stat, nsteps * 2, P, st, g_f64_screen_last, [](const PotrfStep& s, size_t i, const std::vector<int>& h, std::vector<int>& last) {
      if (s.kind == POTRF_UPDATE_LEAF && s.screened) last.insert(last.end(), {s.M, s.N, s.h, h[2 * i], h[2 * i + 1]});
    });
  if (g_zero_ext_stats)          // test hook only
    read_step_counters(zx_stat, nsteps, P, st, g_zero_ext_last, [&](const PotrfStep& s, size_t i, const std::vector<int>& h, std::vector<int>& last) {
      if (s.kind == POTRF_UPDATE_LEAF || s.kind == POTRF_EMUL_UPDATE_LEAF || s.kind == POTRF_REGION)
        last.insert(last.end(), {(int)s.kind, s.j0, s.h, s.N, s.M, h[i], s.kind == POTRF_REGION ? region_n128[i] : (s.fused_bulk ? 1 : 0) + 2 * (int)s.strip});
    });
}

// One matrix: the batch of one
void potrf_one(double* A, int ld, int NR, int NC, double* W, int n_real, int* info, hipStream_t st) {
  Batch B; B.add(A, W, info);
  potrf_batch(B, ld, NR, NC, n_real, st);
}

// R (nr x NC, ldr) <- R * L^-T for an already factored L (ld) with inverse diagonal blocks W.
// tri: R starts as the identity and becomes the upper triangular L^-T; rows below the current column block are still
// zero and are skipped (~n^3/3 flops instead of n^3 for a rectangular solve).
// The same solve for a batch of (R_j, L_j, W_j) of identical shapes in lock-step launches (blockIdx.y = matrix).
// det: no split-K in the updates (bitwise reproducible; the predictive-marginal gradients)
void trsm_rec(const BatchPtr& R, int ldr, int nr, const BatchPtr& L, int ld, const BatchPtr& W, int nb, int j0, int w,
              hipStream_t st, bool tri = false, bool top = true, bool det = false) {
  if (top)
    for (int j = 0; j < nb; ++j) {
      guard_extent(R.p[j], nr, ldr, (size_t)j0 + w, true, "batched triangular solve (R)");
      guard_extent(L.p[j], (size_t)j0 + w, ld, (size_t)j0 + w, true, "batched triangular solve (L)");
      guard_extent(W.p[j], 64, 64, (size_t)((j0 + w) / 64) * 64, true, "batched triangular solve (inverse blocks)");
    }
  if (w <= 64) {
    const int rows = tri ? std::min(nr, j0 + 64) : nr;
    ProfScope ps(LMM_PROF_SOLVE_LEAF, (double)nb * rows * 64.0 * 64.0, st, rows, 64, 64);       // 64-column solve by the inverse block: rows * 64^2 flops
    launch_gemm_nt(R, (size_t)j0 * ldr, ldr, R, (size_t)j0 * ldr, ldr, W, (size_t)(j0 / 64) * 4096, 64, rows, 64, 64, 0, true, nb, st);
    return;
  }
  const int h = split(w);
  trsm_rec(R, ldr, nr, L, ld, W, nb, j0, h, st, tri, false, det);
  const int rows = tri ? std::min(nr, j0 + h) : nr;
  {
    // R[:, j0+h : j0+w] -= R[:, j0 : j0+h] L[j0+h : j0+w, j0 : j0+h]': 2 rows (w - h) h flops; bytes: the target block read + written,
    // both operand blocks read once
    const double r = rows, c = w - h, k = h;
    ProfScope ps(LMM_PROF_SOLVE, (double)nb * 2.0 * r * c * k, st, rows, w - h, h, (double)nb * (16.0 * r * c + 8.0 * r * k + 8.0 * c * k));
    launch_gemm_nt(R, (size_t)(j0 + h) * ldr, ldr, R, (size_t)j0 * ldr, ldr, L, (size_t)j0 * ld + (j0 + h), ld, rows, w - h, h, 0, false,
                   nb, st, det);
  }
  trsm_rec(R, ldr, nr, L, ld, W, nb, j0 + h, w - h, st, tri, false, det);
}

// One matrix: the batch of one (element offsets are applied inside the kernels in units of the storage type, so the solve is
// correct in the fp32 compute mode too -- pointer arithmetic on the opaque double* would not be)
void trsm_rec(double* R, int ldr, int nr, const double* L, int ld, const double* W, int j0, int w, hipStream_t st, bool tri = false) {
  BatchPtr Rb{}, Lb{}, Wb{};
  Rb.p[0] = R; Lb.p[0] = const_cast<double*>(L); Wb.p[0] = const_cast<double*>(W);
  trsm_rec(Rb, ldr, nr, Lb, ld, Wb, 1, j0, w, st, tri);
}

// R (nr x NC, ldr) <- R * L^-1 for an already factored L (ld) with inverse diagonal blocks W, batched as trsm_rec (predictive-marginal
// gradients: W = K(x*, x) K^-1 from the forward path's R = K(x*, x) L^-T).  X L = R is solved from the right: with L = [L11 0; L21 L22]
// on the columns [j0, j0 + w), X2 = R2 L22^-1, then R1 -= X2 L21 (L21 = L[j0+h :, j0 : j0+h] read as it lies: an NN product), then
// X1 = R1 L11^-1; the 64-column leaves are R_J W_J.  n^2 nr flops, the same as the forward solve.
void trsm_right_rec(const BatchPtr& R, int ldr, int nr, const BatchPtr& L, int ld, const BatchPtr& W, int nb, int j0, int w,
                    hipStream_t st, bool top = true) {
  if (top)
    for (int j = 0; j < nb; ++j) {
      guard_extent(R.p[j], nr, ldr, (size_t)j0 + w, true, "batched right triangular solve (R)");
      guard_extent(L.p[j], (size_t)j0 + w, ld, (size_t)j0 + w, true, "batched right triangular solve (L)");
      guard_extent(W.p[j], 64, 64, (size_t)((j0 + w) / 64) * 64, true, "batched right triangular solve (inverse blocks)");
    }
  if (w <= 64) {
    launch_trsm_nn(R, (size_t)j0 * ldr, ldr, R, (size_t)j0 * ldr, ldr, W, (size_t)(j0 / 64) * 4096, 64, nr, 64, 64, true, nb, st);
    return;
  }
  const int h = split(w);
  trsm_right_rec(R, ldr, nr, L, ld, W, nb, j0 + h, w - h, st, false);
  launch_trsm_nn(R, (size_t)j0 * ldr, ldr, R, (size_t)(j0 + h) * ldr, ldr, L, (size_t)j0 * ld + (j0 + h), ld, nr, h, w - h, false, nb, st);
  trsm_right_rec(R, ldr, nr, L, ld, W, nb, j0, h, st, false);
}

// alpha (in place over z = L^-1 delta) <- L^-T z for one factor matrix
void backsolve1(const double* L, int ld, const double* W, int nblk, double* z, hipStream_t st) {
  BatchPtr Lb{}, Wb{}, zb{};
  Lb.p[0] = const_cast<double*>(L); Wb.p[0] = const_cast<double*>(W); zb.p[0] = z;
  launch_backsolve(Lb, ld, Wb, nblk, zb, 1, st);
}

// How many latents share one batch and how many streams carry batches, for a shard of ms latents.
// bytes_per_latent > 0: the working set one latent needs while its batch is in flight; the plan is then shrunk (batch first,
// streams second) until nb_per * nstreams * bytes_per_latent fits in 80 % of the free device memory (+ this library's cache).
void batch_plan(int ms, int* nb_per, int* nstreams_used, double bytes_per_latent = 0.0) {
  static int bmax = -1;
  if (bmax < 0) { const char* e = getenv("LMM_BATCH"); bmax = e ? atoi(e) : 16; if (bmax < 1) bmax = 1; if (bmax > LMM_MAX_BATCH) bmax = LMM_MAX_BATCH; }   // round 2: 16 (C2: 690 vs 696 ms at 8)
  // ONE lock-step batch per `bmax` latents (with the software-pipelined update kernel a fuller batch beats two smaller ones on two
  // streams at every size: C2 share of 4 latents 99.5 ms as one batch, 102.3 as 2 x 2, 105.4 as 4 x 1, round 2); concurrent streams
  // carry the batches of larger shards.
  // small factor matrices (n <= ~2000) are latency-bound end to end: one lock-step batch of up to LMM_MAX_BATCH latents costs the
  // same leaf chain as a batch of 8 (reference notebook shape, 20 latents: 3 batches of 8/8/4 -> one of 20)
  constexpr int bsmall = LMM_MAX_BATCH;
  const int bcap = (bytes_per_latent > 0.0 && bytes_per_latent <= 4e7) ? std::max(bmax, bsmall) : bmax;
  int b = std::min(bcap, std::max(1, ms));
  if (g.prof && g.prof_serial) b = std::min(bcap, ms);  // instrumented pass: production-sized batches on ONE stream
  int nbatches = (ms + b - 1) / b;
  int ns = std::max(1, std::min(nbatches, eff_streams()));
  if ((double)b * ns * bytes_per_latent > 8e9) {      // small working sets never need the (slow) driver query
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
      double avail = (double)fr;
      for (const auto& kv : g.pool) avail += (double)kv.first;
      const double budget = 0.8 * avail;
      // + per stream what the plan's emul_stream_budget sets aside (the emulation block at its cap and the block maxima of all nce
      // columns), for working sets whose matrices have an emulated level at the batch size the plan starts from (emul_view: the plan
      // potrf_batch makes; the shape is the square one of this working set, n = sqrt(bytes / 8) rounded up to whole panels, with one
      // 64-row block of riders)
      const int nce = (int)rup((size_t)std::sqrt(bytes_per_latent / 8.0), 128);
      const double per_stream = g_f32 ? 0.0 : emul_stream_budget(emul_view(nce + 64, nce, b), nce + 64, nce, b);
      while ((double)b * ns * bytes_per_latent + ns * per_stream > budget && (b > 1 || ns > 1)) {
        if (b > 1) b = (b + 1) / 2; else --ns;
        nbatches = (ms + b - 1) / b;
        ns = std::max(1, std::min(ns, nbatches));
      }
    } else (void)hipGetLastError();
  }
  *nb_per = b;
  *nstreams_used = ns;
}

struct Slot {                 // one stream + the factor matrices of the batch it carries
  std::vector<Buf<double>> A, W, R;      // R: optional second matrix per latent (the gradient cores' identity riders -> L^-T)
  Buf<double> part;                      // optional reduction scratch, reused latent after latent in stream order
  hipStream_t st;
};

void make_slots(std::vector<Slot>& slots, int count, int nb_per, size_t a_elems, int NC, size_t r_elems = 0, size_t part_elems = 0) {
  slots.resize(count);
  for (int s = 0; s < count; ++s) {
    for (int j = 0; j < nb_per; ++j) {
      slots[s].A.emplace_back(mat_count(a_elems));
      slots[s].W.emplace_back(mat_count((size_t)(NC / 64) * 4096));
      if (r_elems) slots[s].R.emplace_back(mat_count(r_elems));
    }
    if (part_elems) slots[s].part = Buf<double>(part_elems);
    slots[s].st = g.streams[s];
  }
}

void fork_slots(int count) {       // slot streams wait for everything queued on the main stream
  g_in_flight = count > 1 ? count : 1;
  if (count <= 1) return;          // (one slot = the main stream itself: no event -- a recorded event is a marker packet the queue
                                   // takes microseconds to retire, in front of a small problem's Gram launch)
  HIPCHK(hipEventRecord(g.ev_main, g.streams[0]));
  for (int s = 1; s < count; ++s) HIPCHK(hipStreamWaitEvent(g.streams[s], g.ev_main, 0));
}

void join_slots(int count) {       // main stream waits for every slot stream
  g_in_flight = 1;
  for (int s = 1; s < count; ++s) {
    HIPCHK(hipEventRecord(g.ev_slot[s], g.streams[s]));
    HIPCHK(hipStreamWaitEvent(g.streams[0], g.ev_slot[s], 0));
  }
}

int check_info(const int* info, size_t count, int latent_begin);

// The host-side fan-out every per-latent loop goes through: the ms latents of a shard in batches of nb_per, batch bi on slot stream
// bi % nslots, between fork_slots and join_slots.  It also owns the pivot-info words of the shard's factorisations.
struct FanBatch { int s; hipStream_t st; int k0, nb; };      // slot, its stream, first latent of the batch (shard index), latents in it
struct FanOut {
  int ms, mk;                    // latents of the shard; max(ms, 1), the count the per-latent buffers of a possibly empty shard take
  int nb_per = 1, nslots = 1;
  int* info = nullptr;           // device: info[k] of latent k (alloc_info; or the caller's own words, which the caller then reads back)
  FanOut(int ms_, double bytes_per_latent) : ms(ms_), mk(std::max(ms_, 1)) { batch_plan(mk, &nb_per, &nslots, bytes_per_latent); }
  // the one-slot form: every batch on the main stream, as many latents per batch as one launch takes
  static FanOut one_slot(int ms_) { FanOut F(ms_); F.nb_per = std::min(F.mk, LMM_MAX_BATCH); return F; }
  int* alloc_info(int words_per_latent = 1) {      // zeroed on the main stream, ahead of the fork
    own = Buf<int>((size_t)words_per_latent * mk);
    HIPCHK(hipMemsetAsync(own.p, 0, own.n * sizeof(int), g.streams[0]));
    return info = own.p;
  }
  template <class Body>
  void run(Body&& body) {
    struct Scope {               // the "several batches in flight" state must not outlive the loop, whichever way it is left
      explicit Scope(int count) { fork_slots(count); }
      ~Scope() { g_in_flight = 1; }
    } scope(nslots);
    int bi = 0;
    for (int k0 = 0; k0 < ms; k0 += nb_per, ++bi) {
      const int s = bi % nslots;
      body(FanBatch{s, g.streams[s], k0, std::min(nb_per, ms - k0)});
    }
    join_slots(nslots);
  }
  // After run(): the copy of the info words to the host (main stream), for callers with copies of their own to queue behind it ...
  void fetch_info() {
    hinfo.assign(own.n, 0);
    HIPCHK(hipMemcpyAsync(hinfo.data(), own.p, own.n * sizeof(int), hipMemcpyDeviceToHost, g.streams[0]));
  }
  // ... the words on the host once the main stream has drained, and their status
  const int* host_info() {
    if (hinfo.empty()) fetch_info();
    HIPCHK(hipStreamSynchronize(g.streams[0]));
    return hinfo.data();
  }
  int check(int l0) { return check_info(host_info(), hinfo.size(), l0); }
 private:
  explicit FanOut(int ms_) : ms(ms_), mk(std::max(ms_, 1)) {}
  Buf<int> own;
  std::vector<int> hinfo;
};

// Pivot-info words of a batch -> status.  A dependency-wait timeout of potrf_region_kernel (LMM_INFO_SYNC_TIMEOUT in ANY word) outranks
// a PosDefException in an earlier latent: it means the launch was drained with results undefined, which must never be reported as a
// property of the caller's matrix.  (The abort words the kernel raised are epoch-tagged, so they need no reset: a later launch never
// matches them.)
int check_info(const int* info, size_t count, int latent_begin) {
  for (size_t k = 0; k < count; ++k)
    if (info[k] == LMM_INFO_SYNC_TIMEOUT)
      return fail(LMM_ERR_HIP, "potrf_region_kernel: a dependency wait timed out (latent %d); the grid was drained, results are invalid",
                  latent_begin + (int)k);
  for (size_t k = 0; k < count; ++k)
    if (info[k] != 0) {
      g.err_latent = latent_begin + (int)k;
      g.err_info = info[k];
      return fail(LMM_ERR_NOT_PD, "PosDefException: matrix is not positive definite; Cholesky factorization failed "
                                  "(latent %d, pivot %d)", g.err_latent, g.err_info);
    }
  return LMM_OK;
}
int check_info(const std::vector<int>& info, int latent_begin) { return check_info(info.data(), info.size(), latent_begin); }

// ------------------------------------------------------------------------------------------------
// host-side small dense algebra (m, p <= a few hundred): projections and regulariser scalars
// ------------------------------------------------------------------------------------------------
// reference src/oilmm.jl:20-30:  T = sqrt(S) \ U'  (m x p, column-major), SigmaT = sigma2 ./ S
// T, H: caller's buffers (m p doubles each; may be pinned memory), ST: m.  H by contiguous columns, T (the transposed image) in
// blocks of 16 outputs so that both its reads and its writes stay in a few cache lines: 11 us instead of 90 at p = 600, m = 20
// (the reference notebook's shape, where this host loop was a fifth of the evaluation); same operations, same results.
void project_orthogonal_into(const double* U, const double* S, int p, int m, double s2, double* T, double* ST, double* H) {
  for (int l = 0; l < m; ++l) {
    const double rs = std::sqrt(S[l]);
    ST[l] = s2 / S[l];
    const double* u = U + (size_t)l * p;
    double* h = H + (size_t)l * p;
    for (int o = 0; o < p; ++o) h[o] = u[o] * rs;          // reference src/orthogonal_matrix.jl:27-30
  }
  for (int o0 = 0; o0 < p; o0 += 16) {
    const int o1 = std::min(p, o0 + 16);
    for (int l = 0; l < m; ++l) {
      const double rs = std::sqrt(S[l]);
      const double* u = U + (size_t)l * p;
      for (int o = o0; o < o1; ++o) T[l + (size_t)o * m] = u[o] / rs;
    }
  }
}
void project_orthogonal(const double* U, const double* S, int p, int m, double s2, std::vector<double>& T,
                        std::vector<double>& ST, std::vector<double>& H) {
  T.resize((size_t)m * p); ST.resize(m); H.resize((size_t)p * m);
  project_orthogonal_into(U, S, p, m, s2, T.data(), ST.data(), H.data());
}

bool host_cholesky(std::vector<double>& A, int m) {   // lower, in place, column-major
  for (int j = 0; j < m; ++j) {
    double d = A[j + (size_t)j * m];
    for (int k = 0; k < j; ++k) d -= A[j + (size_t)k * m] * A[j + (size_t)k * m];
    if (!(d > 0.0)) return false;
    d = std::sqrt(d);
    A[j + (size_t)j * m] = d;
    for (int i = j + 1; i < m; ++i) {
      double s = A[i + (size_t)j * m];
      for (int k = 0; k < j; ++k) s -= A[i + (size_t)k * m] * A[j + (size_t)k * m];
      A[i + (size_t)j * m] = s / d;
    }
  }
  return true;
}

// Symmetric eigendecomposition A = Q diag(lam) Q' by cyclic Jacobi (m <= a few hundred; host).  A, Q column-major.
void host_jacobi_eig(std::vector<double> A, int m, std::vector<double>& lam, std::vector<double>& Q) {
  Q.assign((size_t)m * m, 0.0);
  for (int i = 0; i < m; ++i) Q[i + (size_t)i * m] = 1.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < m; ++i) for (int j = 0; j < m; ++j) (i == j ? diag : off) += A[i + (size_t)j * m] * A[i + (size_t)j * m];
    if (off <= 1e-30 * diag) break;
    for (int pi = 0; pi < m - 1; ++pi)
      for (int qi = pi + 1; qi < m; ++qi) {
        const double apq = A[pi + (size_t)qi * m];
        if (apq == 0.0) continue;
        const double theta = (A[qi + (size_t)qi * m] - A[pi + (size_t)pi * m]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < m; ++k) {       // A <- A J
          const double akp = A[k + (size_t)pi * m], akq = A[k + (size_t)qi * m];
          A[k + (size_t)pi * m] = c * akp - s * akq; A[k + (size_t)qi * m] = s * akp + c * akq;
        }
        for (int k = 0; k < m; ++k) {       // A <- J' A
          const double apk = A[pi + (size_t)k * m], aqk = A[qi + (size_t)k * m];
          A[pi + (size_t)k * m] = c * apk - s * aqk; A[qi + (size_t)k * m] = s * apk + c * aqk;
        }
        for (int k = 0; k < m; ++k) {       // Q <- Q J
          const double qkp = Q[k + (size_t)pi * m], qkq = Q[k + (size_t)qi * m];
          Q[k + (size_t)pi * m] = c * qkp - s * qkq; Q[k + (size_t)qi * m] = s * qkp + c * qkq;
        }
      }
  }
  lam.resize(m);
  for (int i = 0; i < m; ++i) lam[i] = A[i + (size_t)i * m];
}

// C (r x c) = op(A) op(B), column-major, op(A) r x k and op(B) k x c; ta / tb: the operand is stored transposed.  Every element is the
// sum over the inner index in ascending order from 0.0: the order the callers' values are pinned in, bit for bit.
std::vector<double> host_matmul(const double* A, bool ta, const double* B, bool tb, int r, int k, int c) {
  std::vector<double> Cm((size_t)r * c, 0.0);
  for (int j = 0; j < c; ++j)
    for (int q = 0; q < k; ++q) {
      const double b = tb ? B[j + (size_t)q * c] : B[q + (size_t)j * k];
      for (int i = 0; i < r; ++i) Cm[i + (size_t)j * r] += (ta ? A[q + (size_t)i * k] : A[i + (size_t)q * r]) * b;
    }
  return Cm;
}

// B (m x nrhs, column-major) <- (L L')^-1 B in place, L the lower factor host_cholesky leaves: forward, then backward substitution
void host_chol_solve(const std::vector<double>& L, int m, double* B, int nrhs) {
  for (int c = 0; c < nrhs; ++c) {
    double* v = B + (size_t)c * m;
    for (int a = 0; a < m; ++a) {
      double s = v[a];
      for (int k = 0; k < a; ++k) s -= L[a + (size_t)k * m] * v[k];
      v[a] = s / L[a + (size_t)a * m];
    }
    for (int a = m - 1; a >= 0; --a) {
      double s = v[a];
      for (int k = a + 1; k < m; ++k) s -= L[k + (size_t)a * m] * v[k];
      v[a] = s / L[a + (size_t)a * m];
    }
  }
}

// reference src/ilmm.jl:61-68: P = H'H / s2 + jitter I, T = P^-1 H' / s2 (m x p), ST = s2 T T' (m x m; all column-major); also
// logdet(ST) for src/ilmm.jl:179.
int project_dense(const double* H, int p, int m, double s2, double jitter, std::vector<double>& T,
                  std::vector<double>& ST, double* logdetST) {
  std::vector<double> G = host_matmul(H, true, H, false, m, p, m);
  for (int a = 0; a < m; ++a)
    for (int b = 0; b < m; ++b) G[a + (size_t)b * m] = G[a + (size_t)b * m] / s2 + (a == b ? jitter : 0.0);
  if (!host_cholesky(G, m)) return fail(LMM_ERR_NOT_PD, "PosDefException in project(H, sigma2): H'H/sigma2 + 1e-9 I not PD");
  T.assign((size_t)m * p, 0.0);
  for (int o = 0; o < p; ++o)
    for (int a = 0; a < m; ++a) T[a + (size_t)o * m] = H[o + (size_t)a * p] / s2;
  host_chol_solve(G, m, T.data(), p);
  ST = host_matmul(T.data(), false, T.data(), true, m, p, m);
  for (double& v : ST) v = s2 * v;
  if (logdetST) {
    std::vector<double> C = ST;
    if (!host_cholesky(C, m)) return fail(LMM_ERR_NOT_PD, "PosDefException: SigmaT not PD");
    double ld = 0.0;
    for (int a = 0; a < m; ++a) ld += std::log(C[a + (size_t)a * m]);
    *logdetST = 2.0 * ld;
  }
  return LMM_OK;
}

// project_dense differentiated, host algebra only: from the cotangents Tb of T and Gs of ST, ADD the cotangent of H (p x m) to Hb and
// that of s2 to s2g.  The caller's own terms are in Hb and s2g before the call, and every sum runs in the order written here: the
// dense-H gradients are pinned bit for bit (tools/bitwise_vs_parent.py).
int project_dense_backward(const double* H, int p, int m, double s2, double jitter, const std::vector<double>& T, std::vector<double> Tb,
                           const std::vector<double>& Gs, std::vector<double>& Hb, double& s2g) {
  const size_t mm = (size_t)m * m;
  const double s = 1.0 / s2;
  const std::vector<double> HtH = host_matmul(H, true, H, false, m, p, m);
  // ST = s2 T T':  Tb += s2 (Gs + Gs') T;  s2g += <Gs, T T'>
  std::vector<double> Gsym(mm), Psym(mm);
  for (int a = 0; a < m; ++a)
    for (int b = 0; b < m; ++b) Gsym[a + (size_t)b * m] = Gs[a + (size_t)b * m] + Gs[b + (size_t)a * m];
  const std::vector<double> GT = host_matmul(Gsym.data(), false, T.data(), false, m, m, p);
  const std::vector<double> TTt = host_matmul(T.data(), false, T.data(), true, m, p, m);
  for (size_t q = 0; q < Tb.size(); ++q) Tb[q] += s2 * GT[q];
  for (int a = 0; a < m; ++a)
    for (int b = 0; b < m; ++b) s2g += Gs[a + (size_t)b * m] * TTt[a + (size_t)b * m];
  // T = P^-1 H' s with P = s H'H + jitter I:  Mb = P^-1 Tb (m x p, in Tb's place);  Pb = -Mb T'
  std::vector<double> P(mm);
  for (int a = 0; a < m; ++a)
    for (int b = 0; b < m; ++b) P[a + (size_t)b * m] = s * HtH[a + (size_t)b * m] + (a == b ? jitter : 0.0);
  if (!host_cholesky(P, m)) return fail(LMM_ERR_NOT_PD, "PosDefException in project(H, sigma2)");
  const std::vector<double>& Mb = Tb;
  host_chol_solve(P, m, Tb.data(), p);
  std::vector<double> Pb = host_matmul(Mb.data(), false, T.data(), true, m, p, m);
  for (double& v : Pb) v = -v;
  for (int a = 0; a < m; ++a)
    for (int b = 0; b < m; ++b) Psym[a + (size_t)b * m] = Pb[a + (size_t)b * m] + Pb[b + (size_t)a * m];
  const std::vector<double> HP = host_matmul(H, false, Psym.data(), false, p, m, m);      // P = s H'H:  Hb += s H (Pb + Pb')
  double sb = 0.0;       // cotangent of s = 1 / s2
  for (int o = 0; o < p; ++o)
    for (int l = 0; l < m; ++l) {
      Hb[o + (size_t)l * p] += s * Mb[l + (size_t)o * m];                        // M = H' s
      sb += Mb[l + (size_t)o * m] * H[o + (size_t)l * p];
      Hb[o + (size_t)l * p] += s * HP[o + (size_t)l * p];
    }
  for (int a = 0; a < m; ++a)
    for (int b = 0; b < m; ++b) sb += Pb[a + (size_t)b * m] * HtH[a + (size_t)b * m];
  s2g += -sb * s * s;
  return LMM_OK;
}

struct Uploaded {   // small host arrays staged on the device
  Buf<double> buf;
  Uploaded() = default;
  // direct_small: up to 256 values that kernels only READ (a few times, as uniform loads) are left in the pinned arena and read
  // from there through its device mapping -- one copy operation less per call, which is ~8 % of a C0-sized evaluation
  Uploaded(const std::vector<double>& v, hipStream_t st, bool direct_small = false) {
    void* pp = pin_take(v.size() * sizeof(double));
    if (pp) std::memcpy(pp, v.data(), v.size() * sizeof(double));
    stage(pp ? static_cast<const double*>(pp) : v.data(), pp != nullptr, v.size(), st, direct_small);
  }
  // values the caller already wrote into the pinned arena (pin_take)
  Uploaded(const double* pinned, size_t count, hipStream_t st, bool direct_small) { stage(pinned, true, count, st, direct_small); }
 private:
  void stage(const double* src, bool pinned, size_t count, hipStream_t st, bool direct_small) {
    if (direct_small && pinned && count <= 256 && g.pin_dev) {
      buf.p = pin_dev(const_cast<double*>(src)); buf.n = count; buf.own = false;
      return;
    }
    buf = Buf<double>(count);
    HIPCHK(hipMemcpyAsync(buf.p, src, count * sizeof(double), hipMemcpyHostToDevice, st));
  }
};

// Ty (n x C, ld n) = In (n x K) * Mx' - sub;  optionally residual sum of squares |Ref - Ty * Hm'|_F^2.
void project_on_device(const double* Y, int n, int p, const double* Td, int m, int c0, int C,
                       const double* sub_dev, double* Ty, hipStream_t st) {
  launch_tall_skinny(Y, n, n, p, Td + c0, m, C, Ty, n, sub_dev, nullptr, 0, nullptr, 0, st);
}
void project_on_device(const double* Y, int n, int p, const Buf<double>& Td, int m, int c0, int C,
                       const double* sub_dev, double* Ty, hipStream_t st) {
  project_on_device(Y, n, p, Td.p, m, c0, C, sub_dev, Ty, st);
}

void residual_on_device(const double* Y, int n, int p, const double* Ty_all, int m, const double* Hd,
                        double* partial, double* out1, hipStream_t st) {
  launch_tall_skinny(Ty_all, n, n, m, Hd, p, p, nullptr, 0, nullptr, Y, n, partial, 1, st);
  launch_sum_partials(partial, tall_skinny_partials(n, p), out1, st);
}
void residual_on_device(const double* Y, int n, int p, const double* Ty_all, int m, const Buf<double>& Hd,
                        double* partial, double* out1, hipStream_t st) {
  residual_on_device(Y, n, p, Ty_all, m, Hd.p, partial, out1, st);
}

// The regulariser of reference src/oilmm.jl:101-113 for n points with noise s2 and resid = |(I - U U') Y|_F^2
double oilmm_regulariser(double n, int p, int m, const double* S, double s2, double resid) {
  double logdetS = 0.0;
  for (int l = 0; l < m; ++l) logdetS += std::log(S[l]);
  return -(n * (logdetS + (double)(p - m) * std::log(2.0 * M_PI * s2)) + resid / s2) / 2.0;
}
// The dense-H one, reference src/ilmm.jl:171-181, for cnt points with noise s2 and resid = |Y - H T Y|_F^2
double ilmm_regulariser(double cnt, int p, int m, double s2, double logdetST, double resid) {
  return -(cnt * ((double)(p - m) * kLog2Pi + ((double)p * std::log(s2) - logdetST)) + resid / s2) / 2.0;
}

// The projection front end of complete data (reference src/oilmm.jl:20-30): T, the projected noise ST and H on the host (the
// constructor); T and the latent means on the device (upload); then, on streams[0], the shard's residual rows (delta) or the plain
// rows of T y with the regulariser's residual (rows).
struct OilmmFront {
  int p, m;
  std::vector<double> T, ST, H;
  Uploaded Td, meansd, Hd;
  Buf<double> Ty, resid_dev, partial;
  OilmmFront(int p_, int m_) : p(p_), m(m_) {}
  OilmmFront(const double* U, const double* S, int p_, int m_, double s2) : p(p_), m(m_) { project_orthogonal(U, S, p, m, s2, T, ST, H); }
  static OilmmFront identity(int m) {      // an IndependentMOGP: T = I over its m outputs (no ST, no H)
    OilmmFront F(m, m);
    F.T.assign((size_t)m * m, 0.0);
    for (int l = 0; l < m; ++l) F.T[l + (size_t)l * m] = 1.0;
    return F;
  }
  void upload(const std::vector<double>& means) { Td = Uploaded(T, g.streams[0]); meansd = Uploaded(means, g.streams[0]); }
  // delta_l = (T y)_l - mean_l for the ms latents from l0 on, [latent][n]
  Buf<double> delta(const double* yd, int n, int l0, int ms) const {
    Buf<double> out((size_t)n * std::max(ms, 1));
    if (ms > 0) project_on_device(yd, n, p, Td.buf, m, l0, ms, meansd.buf.p + l0, out.p, g.streams[0]);
    return out;
  }
  // (T y)_l of the shard without the means (returned, [latent][n]); with_regulariser: of every latent, and |Y - H T Y|_F^2 copied to
  // *resid, which holds it once streams[0] has been synchronised
  const double* rows(const double* yd, int n, int l0, int ms, bool with_regulariser, double* resid) {
    hipStream_t st0 = g.streams[0];
    const int c0 = with_regulariser ? 0 : l0, C = with_regulariser ? m : ms;
    Ty = Buf<double>((size_t)n * std::max(C, 1));
    if (C > 0) project_on_device(yd, n, p, Td.buf, m, c0, C, nullptr, Ty.p, st0);
    if (with_regulariser) {
      Hd = Uploaded(H, st0);
      partial = Buf<double>(tall_skinny_partials(n, p));
      resid_dev = Buf<double>(1);
      residual_on_device(yd, n, p, Ty.p, m, Hd.buf, partial.p, resid_dev.p, st0);
      HIPCHK(hipMemcpyAsync(resid, resid_dev.p, sizeof(double), hipMemcpyDeviceToHost, st0));
    }
    return Ty.p + (size_t)(l0 - c0) * n;
  }
};

// The front end of the dense-H ILMM for one (H, s2, jitter): project(H, s2) on the host (reference src/ilmm.jl:61-68); T on the device
// and, with n_noise > 0 (the points whose residual is taken), SigmaT, H and the residual's buffers (upload); given the latents, also
// their means and, with n_noise > 0, the LatentDev array of a training matrix; then, on streams[0], the projected residuals T y - mean
// (delta) and the regulariser's |Y - H T Y|_F^2 (residual, which leaves T y in Ty).
struct DenseFront {
  const double* H;
  int p, m;
  std::vector<double> T, ST, Hv, means;      // (the host sides of the uploads live as long as the front end)
  std::vector<LatentDev> lat;
  double logdetST = 0.0;
  Uploaded Td, STd, Hd, meansd;
  Buf<LatentDev> latd;
  Buf<double> Ty, partial;
  DenseFront(const double* H_, int p_, int m_) : H(H_), p(p_), m(m_) {}
  int project(double s2, double jitter, bool logdet) { return project_dense(H, p, m, s2, jitter, T, ST, logdet ? &logdetST : nullptr); }
  void upload(const Latent* lts, int n_noise) {
    hipStream_t st0 = g.streams[0];
    const bool noise = n_noise > 0;
    Td = Uploaded(T, st0);
    if (noise) {
      Hv.assign(H, H + (size_t)p * m); STd = Uploaded(ST, st0); Hd = Uploaded(Hv, st0);
      Ty = Buf<double>((size_t)n_noise * m); partial = Buf<double>(tall_skinny_partials(n_noise, p));
    }
    if (!lts) return;
    means = latent_means(lts, m);
    meansd = Uploaded(means, st0);
    if (!noise) return;
    lat.resize(m);
    for (int l = 0; l < m; ++l) lat[l] = lts[l].dense_dev();
    latd = Buf<LatentDev>(m);
    HIPCHK(hipMemcpyAsync(latd.p, lat.data(), m * sizeof(LatentDev), hipMemcpyHostToDevice, st0));
  }
  void delta(const double* yd, int n, double* out) const { project_on_device(yd, n, p, Td.buf, m, 0, m, meansd.buf.p, out, g.streams[0]); }
  void residual(const double* yd, int n, double* resid_dev) {      // n: the n_noise of upload
    project_on_device(yd, n, p, Td.buf, m, 0, m, nullptr, Ty.p, g.streams[0]);
    residual_on_device(yd, n, p, Ty.p, m, Hd.buf, partial.p, resid_dev, g.streams[0]);
  }
};

// The training matrix of the dense-H ILMM as a factor matrix A (D.NR x D.NC, D.ld): blockdiag(K_l(x, x)) + sigmaT (x) I over n points
// and m latents -- sig_idx (device, n of them, or NULL for one block) picks each point's m x m block of sigmaT -- with nrider rider rows,
// m n apart.  The one place that fills a DenseArgs.
void dense_assemble(double* A, const Dims& D, const double* xd, int d, int n, int m, const LatentDev* lat, int has_sum, const double* sigmaT,
                    const int* sig_idx, const double* rider, int nrider, hipStream_t st) {
  DenseArgs a{};
  a.A = A; a.ld = D.ld; a.nrows = D.NR; a.ncols = D.NC; a.x = xd; a.d = d; a.n = n; a.m = m;
  a.lat = lat; a.sigmaT = sigmaT; a.sig_idx = sig_idx; a.rider = rider; a.rider_ld = m * n; a.nrider = nrider; a.has_sum = has_sum;
  launch_dense_assemble(a, st);
}

// One (N x N) factorisation with nrider rider rows, N = m n: the factor matrix A and the inverse diagonal blocks W (its own, or the
// caller's where the factor is kept), the pivot-info word (zeroed on st by the constructor), the Cholesky and, asked for, every rider's log
// marginal likelihood (factor), and at the end of the caller's launches the values back, the stream synchronised and the pivot
// checked (finish).  The caller assembles A in between: dense_assemble, or dense_post_cov_factor.
struct DenseFactor {
  int N;
  Dims D;
  double *A, *W;
  Buf<double> Aown, Wown, lml_dev;
  Buf<int> info;
  DenseFactor(int N_, int nrider, hipStream_t st, double* A_ = nullptr, double* W_ = nullptr)
      : N(N_), D(N_, nrider), A(A_), W(W_), lml_dev(std::max(nrider, 1)), info(1) {
    if (!A) { Aown = Buf<double>(mat_count(D.elems())); A = Aown.p; }
    if (!W) { Wown = Buf<double>(mat_count((size_t)(D.NC / 64) * 4096)); W = Wown.p; }
    HIPCHK(hipMemsetAsync(info.p, 0, sizeof(int), st));
  }
  void factor(bool lml, hipStream_t st) {
    potrf_one(A, D.ld, D.NR, D.NC, W, N, info.p, st);
    if (lml) launch_lml_reduce(A, D.ld, N, D.NC, (int)lml_dev.n, lml_dev.p, st);
  }
  int finish(double* lml, hipStream_t st) {
    int hinfo = 0;
    if (lml) HIPCHK(hipMemcpyAsync(lml, lml_dev.p, lml_dev.n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&hinfo, info.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return check_info(std::vector<int>{hinfo}, 0);
  }
};

// The training matrix of one latent as a factor matrix A (D.NR x D.NC, D.ld): K(x, x) + noise on the diagonal -- the scalar `noise`, or
// the per-point values noisevec (device, n of them) when given -- the identity on the padding, and nrider rider rows (rider, n apart)
// less rider_sub.  info_zero: the matrix's pivot-info word, zeroed by the launch.
GramArgs train_gram_args(const Latent& gp, const double* xd, int d, int n, const Dims& D, double* A, double noise, const double* noisevec,
                         const double* rider, int nrider, double rider_sub = 0.0, int* info_zero = nullptr) {
  GramArgs a{};
  a.A = A; a.ld = D.ld; a.nrows = D.NR; a.ncols = D.NC; a.x = xd; a.d = d; a.n = n;
  gp.set_kernel(a); a.pad_diag = 1.0;
  a.diag_add = noisevec ? 0.0 : noise; a.diag_vec = noisevec;
  a.rider = rider; a.rider_ld = n; a.nrider = nrider; a.rider_sub = rider_sub;
  a.info_zero = info_zero;
  return a;
}
// bytes of the lower triangle a training Gram launch writes (its ProfScope's work and bytes, per latent)
inline double train_gram_bytes(int n) { return (double)n * ((double)n + 1.0) / 2.0 * 8.0; }

// Core: per-latent log marginal likelihoods for latents [l0, l1) given the device rider vectors
// delta ([latent][rhs][n]) and per-latent noise.  Returns lml[latent * nrhs + rhs] (host).  nrhs > 1: several
// right-hand sides (matrix-Y logpdf) ride one factorisation.  noisevec ([latent of the shard][n], device) replaces the
// scalar per-latent noise by a per-point diagonal.
int latent_lmls(const double* xd, int d, int n, const Latent* lts, const double* noise, int l0, int l1,
                const double* delta, std::vector<double>& lml, int nrhs = 1, const double* noisevec = nullptr,
                const double* rider_sub = nullptr,         // rider_sub[latent] (host): subtracted from that latent's riders
                const std::function<void()>* pre_launch = nullptr) {      // launches that PRODUCE delta, issued on streams[0] once this
                                                           // function's host-side preparation is done (see lmm_oilmm_logpdf)
  const int ms = l1 - l0;
  lml.assign((size_t)ms * nrhs, 0.0);
  if (ms == 0) {
    if (pre_launch) (*pre_launch)();
    // callers read pinned results (regulariser residual) and release their device buffers after this returns: the main stream
    // must be drained even when this rank holds no latent
    HIPCHK(hipStreamSynchronize(g.streams[0]));
    return LMM_OK;
  }
  Dims D(n, nrhs);
  FanOut F(ms, mat_bytes((double)D.elems()));
  std::vector<Slot> slots;
  make_slots(slots, F.nslots, F.nb_per, D.elems(), D.NC);
  // results: [ms * nrhs doubles | ms pivot-info ints] in ONE buffer.  When the pinned arena is mapped into the device, lml_reduce
  // writes both straight into host memory (pk) and nothing is copied back; else one copy brings both back.  The pivot-info words
  // the kernels work on are zeroed by each latent's Gram launch (no memset).
  const size_t nout = (size_t)ms * nrhs;
  const size_t nbytes = (nout + ((size_t)ms + 1) / 2) * sizeof(double);
  Buf<double> out(nout + ((size_t)ms + 1) / 2);
  F.info = reinterpret_cast<int*>(out.p + nout);
  std::vector<double> pageable;
  char* pk = static_cast<char*>(pin_take(nbytes));
  char* pk_dev = pin_dev(pk);
  if (!pk) { pageable.resize(nbytes / sizeof(double)); pk = reinterpret_cast<char*>(pageable.data()); }
  // The kernels that produce the riders go out only now: issued before the plan / slot / pool work above, they finished while the
  // host was still preparing and the device then idled ~5 us ahead of the Gram launch (a twentieth of a C0-sized evaluation)
  if (pre_launch) (*pre_launch)();
  F.run([&](const FanBatch& b) {
    Slot& s = slots[b.s];
    Batch B;
    int* zext = nullptr;
    {
    // the batch's Gram launches share one event pair (back-to-back launches: the event overhead is not charged per launch)
    const double gb = train_gram_bytes(n);
    ProfScope ps(LMM_PROF_GRAM, b.nb * gb, s.st, 0, 0, 0, b.nb * gb, b.nb);
    GramArgs ga[LMM_MAX_BATCH];
    // zero extents (lmm_emul.h): this Gram launch writes every entry of the lower triangle of every matrix of the batch, rider and padding
    // rows included, and nothing else writes them before the factorisation
    // (a matrix of at most one region launch's columns is factored by that launch alone: its row tasks are the rider rows, nothing can be
    // void, and the memset and the per-tile reduction would be pure cost on the small shapes)
    // and the size gate: FactorSwitches.zero_extents_min_cols
    if (!(sw_region_cols() > 0 && D.NC <= sw_region_cols()) && D.NC > factor_switches().zero_extents_min_cols) zext = zero_ext_scratch(D.NR, b.nb, s.st);
    for (int j = 0; j < b.nb; ++j) {
      const int k = b.k0 + j;
      // (noisevec: per-point noise of latent k, n device values)
      ga[j] = train_gram_args(lts[l0 + k], xd, d, n, D, s.A[j].p, noisevec ? 0.0 : noise[l0 + k], noisevec ? noisevec + (size_t)k * n : nullptr,
                              delta + (size_t)k * nrhs * n, nrhs, rider_sub ? rider_sub[l0 + k] : 0.0, F.info + k);
      if (zext != nullptr) { ga[j].zext = zext + (size_t)j * zero_ext_ld(D.NR); ga[j].zext_ld = zero_ext_ld(D.NR); }
      B.add(s.A[j].p, s.W[j].p, F.info + k);
    }
    gram_batch_g(ga, b.nb, s.st);       // one launch per run of equal kernel kinds (blockIdx.z = latent)
    }
    potrf_batch(B, D.ld, D.NR, D.NC, n, s.st, D.NC + nrhs, zext);      // the rider rows NC + nrhs .. NR - 1 are zero padding
    if (pk_dev) launch_lml_reduce(B.A, b.nb, D.ld, n, D.NC, nrhs, reinterpret_cast<double*>(pk_dev) + (size_t)b.k0 * nrhs, s.st, &B.info,
                                  reinterpret_cast<int*>(pk_dev + nout * sizeof(double)) + b.k0);
    else launch_lml_reduce(B.A, b.nb, D.ld, n, D.NC, nrhs, out.p + (size_t)b.k0 * nrhs, s.st);
  });
  if (!pk_dev) HIPCHK(hipMemcpyAsync(pk, out.p, nbytes, hipMemcpyDeviceToHost, g.streams[0]));
  HIPCHK(hipStreamSynchronize(g.streams[0]));
  std::memcpy(lml.data(), pk, nout * sizeof(double));
  return check_info(reinterpret_cast<const int*>(pk + nout * sizeof(double)), (size_t)ms, l0);
}

const lmm_jitters_t kDefaultJit = {1e-9, 1e-12, 1e-18};

void drain_after_error() {
  if (g.init) { (void)hipDeviceSynchronize(); (void)hipGetLastError(); }
  // a throw between fork_slots and join_slots must not leave "several batches in flight" behind: the base-case rule of potrf_batch
  // and the ragged-row choice of the update launches read these, so later calls would silently take another launch plan
  g_in_flight = 1;
  if (g.init) strict_ticket_reset();
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// posterior handle
// ------------------------------------------------------------------------------------------------
struct lmm_post {
  int f32 = 0;                // compute dtype the state was built in (its matrices are float buffers when 1)
  int kind = 0;               // 0: per-latent (OILMM / MOGP), 1: dense ILMM
  int n = 0, d = 0, l0 = 0, l1 = 0, m = 0;
  int NC = 0, NR = 0, ld = 0;
  std::shared_ptr<LatentSet> ls;  // all m latents as the handle was built with them (own copy of the factors: tags may go)
  Buf<double> x;              // d x n
  std::vector<Buf<double>> L; // per latent of the shard: factor matrix (NR x NC, ld)
  std::vector<Buf<double>> W; // inverse diagonal blocks
  std::vector<Buf<double>> alpha;     // C \\ delta
  std::vector<Buf<double>> z;         // per latent: L^-1 delta (contiguous copy of the rider row)
  // kept for sequential conditioning: projected residuals (T y)_l - mean_l, [latent of the shard][n], and the projected noise:
  // one scalar per latent after a first conditioning, per-point values ([latent][n]) once batches with different noise mix
  Buf<double> delta_all, noise_all;
  std::vector<double> noise_scalar;
  // dense ILMM (kind 1): L[0] is the (mn) x (mn) factor, alpha[0] the (mn) weights
  int p = 0;
  Buf<double> ddelta;           // (mn): projected residuals [latent][point]  (kept for sequential conditioning)
  std::vector<double> sigs;     // nbatch x (m x m): SigmaT of every conditioning batch (host)
  std::vector<int> sigidx;      // n: batch index of every training point (host)
  std::vector<double> H;        // p x m column-major (host)
  Buf<LatentDev> latd;          // device latent descriptors
  // latent view of a dense-H posterior (lmm_ilmm_post_latent_view): the device state belongs to `base`; this handle only replaces
  // H by I_m (p = m).  `views` counts the views alive on a base handle; destroying a base that still has views defers its release
  // (zombie) until the last view is destroyed.
  lmm_post* base = nullptr;
  int views = 0;
  bool zombie = false;
};
// the handle that owns the device state of a dense-H posterior (itself, or the base of a latent view)
static inline const lmm_post* dense_state(const lmm_post* P) { return P->base ? P->base : P; }

// The preamble of the prediction entry points, which take a posterior handle or (post == NULL) the prior's latents and a shard.
// post_dtype_check comes first in an entry point; post_shard follows the entry point's own argument test: the handle's kind (refused
// with the entry point's own text `other_kind`; nullptr: the entry point has checked it), its m and d (m_fmt: the entry point's wording;
// d_who: nullptr no check here, "" the short message, else the name of the input in the long one), and the shard and latents from the
// handle, or else from the caller's shard and resolve.  The shard's bounds (shard_check) are the caller's next step.
static int post_dtype_check(const lmm_post* post) {
  if (post && post->f32 != g_f32) return fail(LMM_ERR_ARG, "posterior handle was built in the other compute dtype (lmm_set_compute_dtype)");
  return LMM_OK;
}
// The preamble of the dense-H handle's own entry points (lmm_ilmm_post_*): the dtype, `bad` (the entry point's NULL / size test), the
// handle's kind and d, then D, the handle that owns the device state, and the default jitters.
static int dense_post_args(const lmm_post* post, bool bad, int d, const lmm_post*& D, const lmm_jitters_t*& jit) {
  if (int rc = post_dtype_check(post)) return rc;
  if (!post || bad) return fail(LMM_ERR_ARG, "bad arguments");
  if (post->kind != 1) return fail(LMM_ERR_ARG, "not a dense-H ILMM posterior");
  D = dense_state(post);
  if (post->d != d) return fail(LMM_ERR_DIM, "input dimension mismatch");
  if (!jit) jit = &kDefaultJit;
  return LMM_OK;
}
static int post_shard(const lmm_post* P, const char* other_kind, const lmm_gp_t* gps, int m, int d, int latent_begin, int latent_end,
                      Shard& Q, const char* d_who = "", const char* m_fmt = "posterior has %d latents, H has %d") {
  if (P) {
    if (other_kind && P->kind != 0) return fail(LMM_ERR_UNSUPPORTED, "%s", other_kind);
    Q.ls = P->ls;
    if (P->m != m) return fail(LMM_ERR_DIM, m_fmt, P->m, m);
    if (d_who && P->d != d)
      return *d_who ? fail(LMM_ERR_DIM, "input dimension mismatch: posterior has d=%d, %s has d=%d", P->d, d_who, d)
                    : fail(LMM_ERR_DIM, "input dimension mismatch");
  } else if (int rc = resolve(gps, m, d, Q.ls)) return rc;
  Q.set(P ? P->l0 : latent_begin, P ? P->l1 : latent_end);
  return LMM_OK;
}
// H = U sqrt(S) (S == nullptr: U itself, a dense H) of the ms latents from l0 on, p x max(ms, 1) column-major
static std::vector<double> shard_H(const double* U, const double* S, int p, int l0, int ms) {
  std::vector<double> Hs((size_t)p * std::max(ms, 1), 0.0);
  for (int k = 0; k < ms; ++k)
    for (int o = 0; o < p; ++o) Hs[o + (size_t)k * p] = U[o + (size_t)(l0 + k) * p] * (S ? std::sqrt(S[l0 + k]) : 1.0);
  return Hs;
}

#define LMM_TRY try {
// A throw unwinds through Buf destructors, which hand device blocks back to the caching pool while slot streams may still be
// running kernels on them: drain the device before the caller can issue the next call (which could be given those blocks).
#define LMM_CATCH                                   \
  }                                                 \
  catch (int code) { drain_after_error(); return code; }                 \
  catch (const std::exception& e) { drain_after_error(); return fail(LMM_ERR_HIP, "exception: %s", e.what()); }

#define REQUIRE_INIT()                                                           \
  if (!g.init) return fail(LMM_ERR_ARG, "lmm_init() has not been called");      \
  release_call_scratch();                                                        \
  g.pin_off = 0

extern "C" {

int lmm_init(int device) {
  std::lock_guard<std::mutex> lk(g_mu);
  LMM_TRY
  if (g.init) {
    if (g.device == device) return LMM_OK;
    return fail(LMM_ERR_ARG, "already initialised on device %d (one process per GPU)", g.device);
  }
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0) return fail(LMM_ERR_HIP, "no HIP device available (%s)", hipGetErrorString(e));
  if (device < 0 || device >= count) return fail(LMM_ERR_ARG, "device %d out of range (0..%d)", device, count - 1);
  HIPCHK(hipSetDevice(device));
  const char* ns = getenv("LMM_NSTREAMS");
  g.nstreams = ns ? std::max(1, std::min(kMaxStreams, atoi(ns))) : 4;
  for (int s = 0; s < kMaxStreams; ++s) {
    HIPCHK(hipStreamCreateWithFlags(&g.streams[s], hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&g.ev_slot[s], hipEventDisableTiming));
  }
  HIPCHK(hipEventCreateWithFlags(&g.ev_main, hipEventDisableTiming));
  g.pin_cap = 1u << 20;
  if (hipHostMalloc((void**)&g.pin, g.pin_cap, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); g.pin = nullptr; g.pin_cap = 0; }
  g.pin_dev = nullptr;
  {
    static int direct = -1;            // LMM_DIRECT_RESULTS=0: results come back by hipMemcpy (the round-2 path)
    if (direct < 0) { const char* e = getenv("LMM_DIRECT_RESULTS"); direct = e ? (atoi(e) != 0) : 1; }
    void* dp = nullptr;
    if (direct && g.pin && hipHostGetDevicePointer(&dp, g.pin, 0) == hipSuccess) g.pin_dev = static_cast<char*>(dp);
    else (void)hipGetLastError();
  }
  {
    const size_t fi = region_flag_ints(0) * (size_t)LMM_MAX_BATCH * kMaxStreams;
    HIPCHK(hipMalloc((void**)&g.region_flags, fi * sizeof(int)));
    HIPCHK(hipMemset(g.region_flags, 0, fi * sizeof(int)));
    region_flags_register(g.region_flags, fi);
  }
  { const char* e = getenv("LMM_STRICT_PROGRESS"); if (e) g_strict_progress = atoi(e) != 0; }
  g.device = device;
  g.init = true;
  return LMM_OK;
  LMM_CATCH
}

int lmm_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g.init) return LMM_OK;
  (void)hipDeviceSynchronize();
  strict_ticket_reset();
  if (g.comm) { (void)ncclCommDestroy(g.comm); g.comm = nullptr; g.comm_world = 0; }
  if (g.ev_caller) { (void)hipEventDestroy(g.ev_caller); g.ev_caller = nullptr; }
  release_call_scratch();
  if (g.region_flags) { (void)hipFree(g.region_flags); g.region_flags = nullptr; region_flags_register(nullptr, 0); }
  for (auto& kv : g.pool) (void)hipFree(kv.second);
  g.pool.clear();
  for (int s = 0; s < kMaxStreams; ++s) { (void)hipStreamDestroy(g.streams[s]); (void)hipEventDestroy(g.ev_slot[s]); }
  (void)hipEventDestroy(g.ev_main);
  if (g.pin) { (void)hipHostFree(g.pin); g.pin = nullptr; g.pin_cap = 0; g.pin_dev = nullptr; }
  g.init = false;
  return LMM_OK;
}

const char* lmm_last_error_string(void) { return g.err.c_str(); }

// ---- ARD registry (host only): the message of a refusal is recorded only when the context lock is free at that moment ----------
static int ard_fail(int code, const char* msg) {
  std::unique_lock<std::mutex> lk(g_mu, std::try_to_lock);
  if (lk.owns_lock()) fail(code, "%s", msg);
  return code;
}

// Registers a validated tag (d = 0, ard unused: no factors; alpha = 0: no RQ shape).
static int tag_register(int d, const double* ard, double alpha, int* tag, const char* full_msg, double rho = 0.0, double decay = 0.0,
                        double quality = 0.0) {
  std::lock_guard<std::mutex> lk(g_ard_mu);
  if (g_ard_tags.size() >= LMM_ARD_MAX_TAGS) return ard_fail(LMM_ERR_UNSUPPORTED, full_msg);
  while (g_ard_tags.count(g_ard_next)) g_ard_next = g_ard_next % ((1 << 23) - 1) + 1;     // tag << 8 stays a positive int
  const int t = g_ard_next;
  g_ard_next = g_ard_next % ((1 << 23) - 1) + 1;
  ArdTag& a = g_ard_tags[t];
  a.d = d; a.ard.assign(ard, ard + d); a.grad.assign(d, 0.0); a.alpha = alpha; a.rho = rho; a.decay = decay; a.quality = quality;
  *tag = t;
  return LMM_OK;
}

int lmm_ard_create(int d, const double* lengthscale, int* tag) {
  if (d <= 0 || !lengthscale || !tag) return ard_fail(LMM_ERR_ARG, "lmm_ard_create: bad arguments");
  for (int k = 0; k < d; ++k)
    if (!(lengthscale[k] > 0.0) || !std::isfinite(lengthscale[k])) return ard_fail(LMM_ERR_ARG, "lmm_ard_create: lengthscales must be finite and > 0");
  return tag_register(d, lengthscale, 0.0, tag, "lmm_ard_create: too many live ARD tags");
}

int lmm_kernel_tag_create(int d, const double* ard, double alpha, int* tag) {
  if (d < 0 || !tag || (d == 0) != (ard == nullptr)) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_create: bad arguments");
  if (!(alpha == 0.0 || (alpha > 0.0 && std::isfinite(alpha))))
    return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_create: alpha must be 0 (none) or finite and > 0");
  if (d == 0 && alpha == 0.0) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_create: a tag needs factors or an alpha");
  for (int k = 0; k < d; ++k)
    if (!(ard[k] > 0.0) || !std::isfinite(ard[k])) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_create: factors must be finite and > 0");
  return tag_register(d, ard, alpha, tag, "lmm_kernel_tag_create: too many live tags");
}

int lmm_kernel_tag_create_periodic(int d, const double* ard, double rho, int* tag) {
  if (d < 0 || !tag || (d == 0) != (ard == nullptr)) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_create_periodic: bad arguments");
  if (!(rho > 0.0 && std::isfinite(rho))) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_create_periodic: rho must be finite and > 0");
  for (int k = 0; k < d; ++k)
    if (!(ard[k] > 0.0) || !std::isfinite(ard[k])) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_create_periodic: factors must be finite and > 0");
  return tag_register(d, ard, 0.0, tag, "lmm_kernel_tag_create_periodic: too many live tags", rho);
}

int lmm_kernel_tag_create_locally_periodic(int d, const double* ard, double rho, double decay, int* tag) {
  if (d < 0 || !tag || (d == 0) != (ard == nullptr)) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_create_locally_periodic: bad arguments");
  if (!(rho > 0.0 && std::isfinite(rho))) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_create_locally_periodic: rho must be finite and > 0");
  if (!(decay > 0.0 && std::isfinite(decay))) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_create_locally_periodic: decay must be finite and > 0");
  for (int k = 0; k < d; ++k)
    if (!(ard[k] > 0.0) || !std::isfinite(ard[k])) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_create_locally_periodic: factors must be finite and > 0");
  return tag_register(d, ard, 0.0, tag, "lmm_kernel_tag_create_locally_periodic: too many live tags", rho, decay);
}

int lmm_kernel_tag_create_sho(double quality, int* tag) {
  if (!tag) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_create_sho: bad arguments");
  if (!(quality > 0.5 && std::isfinite(quality))) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_create_sho: quality must be finite and > 1/2 (underdamped)");
  return tag_register(0, nullptr, 0.0, tag, "lmm_kernel_tag_create_sho: too many live tags", 0.0, 0.0, quality);
}

// Registers a validated sum tag; the caller holds g_ard_mu.
static int sum_register(int nterms, const lmm_gp_t* terms, int* tag, bool statespace, const char* full_msg) {
  if (g_ard_tags.size() >= LMM_ARD_MAX_TAGS) return ard_fail(LMM_ERR_UNSUPPORTED, full_msg);
  while (g_ard_tags.count(g_ard_next)) g_ard_next = g_ard_next % ((1 << 23) - 1) + 1;
  const int t = g_ard_next;
  g_ard_next = g_ard_next % ((1 << 23) - 1) + 1;
  ArdTag& a = g_ard_tags[t];
  a.d = 0;
  a.terms.assign(terms, terms + nterms);
  a.tgrad.assign(nterms, lmm_gp_grad_t{0.0, 0.0, 0.0});
  a.statespace = statespace;
  *tag = t;
  return LMM_OK;
}

int lmm_kernel_sum_create(int nterms, const lmm_gp_t* terms, int* tag) {
  if (nterms < 1 || nterms > LMM_SUM_MAX_TERMS || !terms || !tag)
    return ard_fail(LMM_ERR_ARG, "lmm_kernel_sum_create: nterms must be 1..4, terms and tag non-NULL");
  for (int c = 0; c < nterms; ++c) {
    const int base = terms[c].kind & LMM_KERNEL_BASE_MASK;
    if (terms[c].kind < 0 || !base_kind_ok(base))
      return ard_fail(LMM_ERR_UNSUPPORTED, "lmm_kernel_sum_create: a term must have a base kind 0..4, 7 or 10 (sums do not nest)");
    if (!(terms[c].variance > 0.0) || !std::isfinite(terms[c].variance) || !(terms[c].lengthscale > 0.0) ||
        !std::isfinite(terms[c].lengthscale) || terms[c].mean != 0.0)
      return ard_fail(LMM_ERR_ARG, "lmm_kernel_sum_create: a term needs finite variance > 0, lengthscale > 0 and mean 0");
  }
  std::lock_guard<std::mutex> lk(g_ard_mu);
  for (int c = 0; c < nterms; ++c) {
    const int tt = terms[c].kind >> 8;
    if (tt == 0) continue;
    auto it = g_ard_tags.find(tt);
    if (it == g_ard_tags.end() || !it->second.terms.empty())
      return ard_fail(LMM_ERR_ARG, "lmm_kernel_sum_create: a term names an unknown tag or a sum tag");
    if (it->second.alpha > 0.0 && (terms[c].kind & LMM_KERNEL_BASE_MASK) != LMM_KERNEL_RQ)
      return ard_fail(LMM_ERR_ARG, "lmm_kernel_sum_create: a term's tag carries an RQ shape but its kind is not LMM_KERNEL_RQ");
    if (!tag_shape_fits(terms[c].kind & LMM_KERNEL_BASE_MASK, 0.0, it->second.rho, it->second.decay))
      return ard_fail(LMM_ERR_ARG, "lmm_kernel_sum_create: a term's tag carries a rho (or a rho and a decay) its kind does not take");
    if (it->second.quality > 0.0)
      return ard_fail(LMM_ERR_ARG, "lmm_kernel_sum_create: a term's tag carries an SHO quality, which no term kind takes");
  }
  return sum_register(nterms, terms, tag, false, "lmm_kernel_sum_create: too many live tags");
}

// The sum tag of a latent the state-space entry points serve (include/lmm_hip.h "state space: sum latents"): exactly two terms, each a
// plain Matern12 / 32 / 52 (no tag) or an SHO (kind 12; its tag, if any, a quality tag), with state dimensions adding up to at most 4.
int lmm_kernel_sum_create_statespace(int nterms, const lmm_gp_t* terms, int* tag) {
  if (nterms < 1 || !terms || !tag) return ard_fail(LMM_ERR_ARG, "lmm_kernel_sum_create_statespace: nterms must be >= 1, terms and tag non-NULL");
  if (nterms != 2) return ard_fail(LMM_ERR_UNSUPPORTED, "lmm_kernel_sum_create_statespace: the state-space path serves sums of exactly two terms");
  int model[2];
  for (int c = 0; c < nterms; ++c) {
    model[c] = terms[c].kind < 0 ? 0 : ss_model_of(terms[c].kind & LMM_KERNEL_BASE_MASK);
    if (model[c] == 0)
      return ard_fail(LMM_ERR_UNSUPPORTED, "lmm_kernel_sum_create_statespace: a term must be Matern12, Matern32, Matern52 or SHO (kinds 3, 1, 2, 12)");
    if ((terms[c].kind >> 8) != 0 && model[c] != SS_MODEL_SHO)
      return ard_fail(LMM_ERR_UNSUPPORTED, "lmm_kernel_sum_create_statespace: a Matern term takes no tag (per-dimension lengthscales are not served)");
    if (!(terms[c].variance > 0.0) || !std::isfinite(terms[c].variance) || !(terms[c].lengthscale > 0.0) ||
        !std::isfinite(terms[c].lengthscale) || terms[c].mean != 0.0)
      return ard_fail(LMM_ERR_ARG, "lmm_kernel_sum_create_statespace: a term needs finite variance > 0, lengthscale > 0 and mean 0");
  }
  if (ss_pair_model(model[0], model[1], nullptr) == 0)
    return ard_fail(LMM_ERR_UNSUPPORTED, "lmm_kernel_sum_create_statespace: the terms' state dimensions add up to more than 4");
  std::lock_guard<std::mutex> lk(g_ard_mu);
  for (int c = 0; c < nterms; ++c) {
    const int tt = terms[c].kind >> 8;
    if (tt == 0) continue;
    auto it = g_ard_tags.find(tt);
    if (it == g_ard_tags.end() || !(it->second.quality > 0.0))
      return ard_fail(LMM_ERR_ARG, "lmm_kernel_sum_create_statespace: an SHO term's tag must be a live quality tag (lmm_kernel_tag_create_sho)");
  }
  return sum_register(nterms, terms, tag, true, "lmm_kernel_sum_create_statespace: too many live tags");
}

int lmm_kernel_sum_grad(int tag, lmm_gp_grad_t* out) {
  if (!out) return ard_fail(LMM_ERR_ARG, "lmm_kernel_sum_grad: out is NULL");
  std::lock_guard<std::mutex> lk(g_ard_mu);
  auto it = g_ard_tags.find(tag);
  if (it == g_ard_tags.end() || it->second.terms.empty()) return ard_fail(LMM_ERR_ARG, "lmm_kernel_sum_grad: unknown sum tag");
  std::copy(it->second.tgrad.begin(), it->second.tgrad.end(), out);
  return LMM_OK;
}

int lmm_kernel_tag_alpha_grad(int tag, double* out) {
  if (!out) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_alpha_grad: out is NULL");
  std::lock_guard<std::mutex> lk(g_ard_mu);
  auto it = g_ard_tags.find(tag);
  if (it == g_ard_tags.end()) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_alpha_grad: unknown tag");
  if (it->second.rho > 0.0) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_alpha_grad: the tag carries a periodic rho, not an alpha");
  if (it->second.quality > 0.0) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_alpha_grad: the tag carries an SHO quality, not an alpha");
  *out = it->second.galpha;
  return LMM_OK;
}

int lmm_kernel_tag_rho_grad(int tag, double* out) {
  if (!out) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_rho_grad: out is NULL");
  std::lock_guard<std::mutex> lk(g_ard_mu);
  auto it = g_ard_tags.find(tag);
  if (it == g_ard_tags.end() || !(it->second.rho > 0.0)) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_rho_grad: unknown tag, or a tag without a rho");
  *out = it->second.grho;
  return LMM_OK;
}

int lmm_kernel_tag_decay_grad(int tag, double* out) {
  if (!out) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_decay_grad: out is NULL");
  std::lock_guard<std::mutex> lk(g_ard_mu);
  auto it = g_ard_tags.find(tag);
  if (it == g_ard_tags.end() || !(it->second.decay > 0.0)) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_decay_grad: unknown tag, or a tag without a decay");
  *out = it->second.gdecay;
  return LMM_OK;
}

int lmm_kernel_tag_quality_grad(int tag, double* out) {
  if (!out) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_quality_grad: out is NULL");
  std::lock_guard<std::mutex> lk(g_ard_mu);
  auto it = g_ard_tags.find(tag);
  if (it == g_ard_tags.end() || !(it->second.quality > 0.0)) return ard_fail(LMM_ERR_ARG, "lmm_kernel_tag_quality_grad: unknown tag, or a tag without a quality");
  *out = it->second.gquality;
  return LMM_OK;
}

int lmm_ard_destroy(int tag) {
  std::lock_guard<std::mutex> lk(g_ard_mu);
  if (g_ard_tags.erase(tag) == 0) return ard_fail(LMM_ERR_ARG, "lmm_ard_destroy: unknown ARD tag");
  return LMM_OK;
}

int lmm_ard_grad(int tag, double* out) {
  if (!out) return ard_fail(LMM_ERR_ARG, "lmm_ard_grad: out is NULL");
  std::lock_guard<std::mutex> lk(g_ard_mu);
  auto it = g_ard_tags.find(tag);
  if (it == g_ard_tags.end()) return ard_fail(LMM_ERR_ARG, "lmm_ard_grad: unknown ARD tag");
  std::copy(it->second.grad.begin(), it->second.grad.end(), out);
  return LMM_OK;
}

int lmm_last_error_detail(int* latent, int* info) {
  if (latent) *latent = g.err_latent;
  if (info) *info = g.err_info;
  return LMM_OK;
}

int lmm_release_cached_memory(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  (void)hipDeviceSynchronize();
  for (auto& kv : g.pool) (void)hipFree(kv.second);
  g.pool.clear();
  return LMM_OK;
}

int lmm_stream_wait_caller(void* hip_stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!g.ev_caller) HIPCHK(hipEventCreateWithFlags(&g.ev_caller, hipEventDisableTiming));
  HIPCHK(hipEventRecord(g.ev_caller, static_cast<hipStream_t>(hip_stream)));
  HIPCHK(hipStreamWaitEvent(g.streams[0], g.ev_caller, 0));      // slot streams fork from streams[0] (fork_slots)
  return LMM_OK;
  LMM_CATCH
}

// ---- RCCL (the ONE exchange step of the sharded paths) -------------------------------------------
#define NCCLCHK(expr)                                                                                  \
  do {                                                                                                 \
    ncclResult_t r_ = (expr);                                                                          \
    if (r_ != ncclSuccess) throw fail(LMM_ERR_RCCL, "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r_), __FILE__, __LINE__); \
  } while (0)

int lmm_comm_get_unique_id(void* id_out) {
  std::lock_guard<std::mutex> lk(g_mu);
  LMM_TRY
  if (!id_out) return fail(LMM_ERR_ARG, "id_out is NULL");
  static_assert(sizeof(ncclUniqueId) == LMM_UNIQUE_ID_BYTES, "LMM_UNIQUE_ID_BYTES must match ncclUniqueId");
  ncclUniqueId id;
  NCCLCHK(ncclGetUniqueId(&id));
  std::memcpy(id_out, &id, sizeof id);
  return LMM_OK;
  LMM_CATCH
}

int lmm_comm_init_rank(const void* id, int rank, int world) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!id || world < 1 || rank < 0 || rank >= world) return fail(LMM_ERR_ARG, "bad arguments");
  if (g.comm) return fail(LMM_ERR_ARG, "a communicator already exists (rank %d of %d): lmm_comm_destroy first", g.comm_rank, g.comm_world);
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof uid);
  HIPCHK(hipSetDevice(g.device));
  NCCLCHK(ncclCommInitRank(&g.comm, world, uid, rank));
  g.comm_rank = rank; g.comm_world = world;
  return LMM_OK;
  LMM_CATCH
}

int lmm_comm_info(int* rank, int* world) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (rank) *rank = g.comm ? g.comm_rank : 0;
  if (world) *world = g.comm ? g.comm_world : 0;
  return LMM_OK;
}

static int allreduce_f64(double* buf, size_t count, ncclRedOp_t op) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!g.comm) return fail(LMM_ERR_ARG, "no communicator: call lmm_comm_init_rank first");
  if (count == 0) return LMM_OK;
  if (!buf) return fail(LMM_ERR_ARG, "buf is NULL");
  hipStream_t st0 = g.streams[0];
  if (is_device_ptr(buf)) {
    NCCLCHK(ncclAllReduce(buf, buf, count, ncclDouble, op, g.comm, st0));
    HIPCHK(hipStreamSynchronize(st0));
    return LMM_OK;
  }
  // host buffer: stage through the pinned arena when it fits (the scalar logpdf sum always does)
  Buf<double> dev(count);
  double* pin = static_cast<double*>(pin_take(count * sizeof(double)));
  if (pin) std::memcpy(pin, buf, count * sizeof(double));
  HIPCHK(hipMemcpyAsync(dev.p, pin ? pin : buf, count * sizeof(double), hipMemcpyHostToDevice, st0));
  NCCLCHK(ncclAllReduce(dev.p, dev.p, count, ncclDouble, op, g.comm, st0));
  HIPCHK(hipMemcpyAsync(pin ? pin : buf, dev.p, count * sizeof(double), hipMemcpyDeviceToHost, st0));
  HIPCHK(hipStreamSynchronize(st0));
  if (pin) std::memcpy(buf, pin, count * sizeof(double));
  return LMM_OK;
  LMM_CATCH
}
int lmm_allreduce_sum_f64(double* buf, size_t count) { return allreduce_f64(buf, count, ncclSum); }
int lmm_allreduce_max_f64(double* buf, size_t count) { return allreduce_f64(buf, count, ncclMax); }

int lmm_comm_destroy(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  LMM_TRY
  if (g.comm) {
    if (g.init) (void)hipDeviceSynchronize();
    NCCLCHK(ncclCommDestroy(g.comm));
    g.comm = nullptr; g.comm_world = 0; g.comm_rank = 0;
  }
  return LMM_OK;
  LMM_CATCH
}

int lmm_set_compute_dtype(int dtype) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (dtype != LMM_F64 && dtype != LMM_F32) return fail(LMM_ERR_ARG, "dtype must be LMM_F64 or LMM_F32");
  g_f32 = (dtype == LMM_F32) ? 1 : 0;
  return LMM_OK;
}
int lmm_get_compute_dtype(void) { return g_f32 ? LMM_F32 : LMM_F64; }

// Strict forward progress of the dataflow kernels (include/lmm_hip.h, conventions): tasks by arrival ticket instead of blockIdx.x.
int lmm_set_strict_progress(int on) {
  std::lock_guard<std::mutex> lk(g_mu);
  g_strict_progress = on ? 1 : 0;
  return LMM_OK;
}
int lmm_get_strict_progress(void) { return g_strict_progress; }
// test hook: the strict build's workgroups ask for their task indices in reverse order (include/lmm_hip.h)
int lmm_dev_claim_scramble(int on) {
  std::lock_guard<std::mutex> lk(g_mu);
  g_claim_scramble = on ? 1 : 0;
  return LMM_OK;
}

int lmm_set_projection_dtype(int dtype) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (dtype != LMM_PROJ_NATIVE && dtype != LMM_PROJ_BF16 && dtype != LMM_PROJ_BF16X2)
    return fail(LMM_ERR_ARG, "projection dtype must be LMM_PROJ_NATIVE, LMM_PROJ_BF16 or LMM_PROJ_BF16X2");
  g_proj = dtype;
  return LMM_OK;
}
int lmm_get_projection_dtype(void) { return g_proj; }

int lmm_device_synchronize(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  HIPCHK(hipDeviceSynchronize());
  return LMM_OK;
  LMM_CATCH
}

// reference src/orthogonal_matrix.jl:21-23: isapprox(U'U, I) (Frobenius norm, rtol = sqrt(eps)).
int lmm_orthogonal_validate(const double* U, int p, int m) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!U || p <= 0 || m <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  double diff2 = 0.0, g2 = 0.0;
  for (int a = 0; a < m; ++a)
    for (int b = 0; b < m; ++b) {
      double s = 0.0;
      for (int o = 0; o < p; ++o) s += U[o + (size_t)a * p] * U[o + (size_t)b * p];
      g2 += s * s;
      const double dlt = s - (a == b ? 1.0 : 0.0);
      diff2 += dlt * dlt;
    }
  const double rtol = std::sqrt(2.220446049250313e-16);
  if (!(std::sqrt(diff2) <= rtol * std::max(std::sqrt(g2), std::sqrt((double)m))))
    return fail(LMM_ERR_NOT_ORTHOGONAL, "`U` is not an orthogonal matrix");
  return LMM_OK;
}

int lmm_oilmm_logpdf(const double* x, int d, int n, const double* y, int p, const double* U, const double* S, int m,
                     double sigma2, const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser,
                     double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  // (this entry point is tuned to the microsecond at C0 size: it takes the preamble's pieces around its own staging, in its own order)
  Train R;
  if (int rc = train_args(!x || !y || !U || !S || !out || d <= 0 || n <= 0 || p <= 0 || m <= 0, p, m, S, sigma2, latent_begin, latent_end, 0)) return rc;
  if (int rc = train_resolve(gps, m, d, latent_begin, latent_end, R)) return rc;
  if (!(sigma2 > 0.0)) return fail(LMM_ERR_ARG, "sigma2 must be > 0");
  hipStream_t st0 = g.streams[0];
  OilmmFront F(p, m);
  std::vector<double>&T = F.T, &ST = F.ST, &H = F.H;      // (T and H stay empty when the arena holds them)
  // [T | H] straight into the pinned arena when the regulariser path (which uploads both as one block) has room there
  double* packp = with_regulariser ? static_cast<double*>(pin_take(2 * (size_t)m * p * sizeof(double))) : nullptr;
  if (packp) { ST.resize(m); project_orthogonal_into(U, S, p, m, sigma2, packp, ST.data(), packp + (size_t)m * p); }
  else project_orthogonal(U, S, p, m, sigma2, T, ST, H);
  R.upload(x, (size_t)d * n, y, (size_t)n * p);
  const int l0 = R.l0, l1 = R.l1, ms = R.ms;
  double resid_pageable = 0.0;
  double* resid = static_cast<double*>(pin_take(sizeof(double)));      // pinned: the read-back below does not stall the host
  if (resid == nullptr) resid = &resid_pageable;
  *resid = 0.0;
  std::vector<double> lml;
  if (with_regulariser) {
    // ONE upload [T | H]; ONE projection T*Y of all m latents serves the regulariser's residual and, through rider rows that
    // subtract the latent mean inside the Gram kernel, the per-latent right-hand sides delta_l = (T y)_l - mean_l
    std::vector<double> pack;
    if (!packp) { pack = T; pack.insert(pack.end(), H.begin(), H.end()); }
    Uploaded THd = packp ? Uploaded(packp, 2 * (size_t)m * p, st0, true) : Uploaded(pack, st0, true);
    const double* Tdev = THd.buf.p;
    const double* Hdev = THd.buf.p + (size_t)m * p;
    Buf<double> Ty((size_t)n * m), resid_dev(1), partial(tall_skinny_partials(n, p));
    double* resid_direct = (resid != &resid_pageable) ? pin_dev(resid) : nullptr;      // the reduction writes into host memory
    const std::function<void()> produce = [&]() {
      project_on_device(R.yd.p, n, p, Tdev, m, 0, m, nullptr, Ty.p, st0);
      // reference src/oilmm.jl:112: sum(abs2, (I - U U') Y)  ==  |Y - H T Y|_F^2 since H T = U U'
      residual_on_device(R.yd.p, n, p, Ty.p, m, Hdev, partial.p, resid_direct ? resid_direct : resid_dev.p, st0);
      if (!resid_direct) HIPCHK(hipMemcpyAsync(resid, resid_dev.p, sizeof(double), hipMemcpyDeviceToHost, st0));    // read after latent_lmls' sync
    };
    if (int rc = latent_lmls(R.xd.p, d, n, R.lts, ST.data(), l0, l1, Ty.p + (size_t)l0 * n, lml, 1, nullptr, R.means.data(), &produce)) return rc;
  } else {
    F.upload(R.means);
    Buf<double> delta = F.delta(R.yd.p, n, l0, ms);
    if (int rc = latent_lmls(R.xd.p, d, n, R.lts, ST.data(), l0, l1, delta.p, lml)) return rc;
  }
  double total = 0.0;
  for (int k = 0; k < ms; ++k) total += lml[k];
  if (with_regulariser) total += oilmm_regulariser(n, p, m, S, sigma2, *resid);
  *out = total;
  return LMM_OK;
  LMM_CATCH
}

}  // extern "C"

namespace {

NoiseBlocks one_noise_block(int n, double s2) {
  NoiseBlocks nb{};
  nb.nblk = 1; nb.off[0] = 0; nb.off[1] = n; nb.s2[0] = s2;
  return nb;
}
// the conditioning batches (batch_n[b] points with variance batch_s2[b]), optionally followed by ns test points with variance s2s
NoiseBlocks batch_noise_blocks(const int* batch_n, const double* batch_s2, int nbatch, int ns, double s2s) {
  NoiseBlocks nb{};
  nb.off[0] = 0;
  for (int b = 0; b < nbatch; ++b) { nb.off[b + 1] = nb.off[b] + batch_n[b]; nb.s2[b] = batch_s2[b]; }
  nb.nblk = nbatch;
  if (ns > 0) { nb.off[nbatch + 1] = nb.off[nbatch] + ns; nb.s2[nbatch] = s2s; nb.nblk = nbatch + 1; }
  return nb;
}
// argument checks shared by the two *_post_logpdf_grad_seq entries; n = total number of conditioning points
int check_batches(const int* batch_n, const double* batch_s2, int nbatch, int n) {
  if (!batch_n || !batch_s2 || nbatch < 1) return fail(LMM_ERR_ARG, "bad arguments");
  if (nbatch > LMM_MAX_NOISE_BLOCKS - 1) return fail(LMM_ERR_UNSUPPORTED, "more than 7 conditioning batches with their own noise variance");
  long long tot = 0;
  for (int b = 0; b < nbatch; ++b) {
    if (batch_n[b] <= 0) return fail(LMM_ERR_ARG, "empty conditioning batch");
    if (!(batch_s2[b] > 0.0)) return fail(LMM_ERR_ARG, "sigma2 must be > 0");
    tot += batch_n[b];
  }
  if (tot != n) return fail(LMM_ERR_ARG, "batch sizes do not add up to n");
  return LMM_OK;
}

struct OilmmGrad {          // host results of an OILMM gradient (partial sums over the latent shard)
  double value = 0.0;
  std::vector<double> gs2;    // one per noise block
  std::vector<double> gS, gU;
  std::vector<lmm_gp_grad_t> ggps;
  std::vector<double> trec;   // m x LMM_SUM_MAX_TERMS records per latent and term (grad_finish), zeros elsewhere
  void size(int m, int p, int nblk, int d) {      // every sum at zero
    gs2.assign(nblk, 0.0);
    gS.assign(m, 0.0); gU.assign((size_t)p * m, 0.0);
    ggps.assign(m, lmm_gp_grad_t{0.0, 0.0, 0.0});
    trec.assign((size_t)m * LMM_SUM_MAX_TERMS * term_grad_stride(d), 0.0);
  }
};

// The regulariser of reference src/oilmm.jl:101-113, once per noise block: its value (added to `total`), its share of d/dS, d/dU and
// d/dsigma2 (added to G) and PtP = P'P for its d/dY.  M2all: Y Y' (p x p) per noise block.
void oilmm_regulariser_grad(const double* U, const double* S, int p, int m, const NoiseBlocks& NB, const std::vector<double>& M2all,
                            double& total, OilmmGrad& G, std::vector<double>& PtP) {
  const int nblk = NB.nblk;
  const size_t pp = (size_t)p * p;
  std::vector<double> Pm((size_t)p * p, 0.0);
  for (int a1 = 0; a1 < p; ++a1)
    for (int b1 = 0; b1 < p; ++b1) {
      double s = (a1 == b1) ? 1.0 : 0.0;
      for (int l = 0; l < m; ++l) s -= U[a1 + (size_t)l * p] * U[b1 + (size_t)l * p];
      Pm[a1 + (size_t)b1 * p] = s;
    }
  PtP = host_matmul(Pm.data(), false, Pm.data(), false, p, p, p);      // P symmetric: P'P = P P
  const std::vector<double> PU = host_matmul(Pm.data(), false, U, false, p, p, m);
  for (int blk = 0; blk < nblk; ++blk) {                        // reference src/oilmm.jl:101-113, once per noise block
    const double* M2 = M2all.data() + pp * blk;
    const double s2 = NB.s2[blk], cnt = NB.count(blk);
    double Rn = 0.0;                                           // |P Y|_F^2 = tr(P'P Y Y')
    for (int a1 = 0; a1 < p; ++a1) for (int b1 = 0; b1 < p; ++b1) Rn += PtP[a1 + (size_t)b1 * p] * M2[b1 + (size_t)a1 * p];
    total += oilmm_regulariser(cnt, p, m, S, s2, Rn);
    for (int l = 0; l < m; ++l) G.gS[l] += -cnt / (2.0 * S[l]);
    G.gs2[blk] += -0.5 * (cnt * (double)(p - m) / s2 - Rn / (s2 * s2));
    const std::vector<double> M2U = host_matmul(M2, false, U, false, p, p, m);
    const std::vector<double> t1 = host_matmul(Pm.data(), false, M2U.data(), false, p, p, m), t2 = host_matmul(M2, false, PU.data(), false, p, p, m);
    for (size_t q = 0; q < G.gU.size(); ++q) G.gU[q] += (t1[q] + t2[q]) / s2;
  }
}

// The back end of the OILMM gradients for complete data (oilmm_grad_core, sparse_oilmm_grad, ss_logpdf_grad): the chain rule from a
// path's per-latent sensitivities back through r_l = (T y)_l - mean_l with T = S^-1/2 U', the projected noise s2[b] / S_l and the
// regulariser, into G.gs2 / gS / gU and d/dY.  The latents' own (variance, lengthscale, mean) gradients stay with the paths.
struct OilmmGradIn {      // what a path hands it; the first row is set by position, the rest by name
  const double* yd; int n, p; const double *U, *S; int m; NoiseBlocks NB; int l0, l1, with_regulariser;
  // a (device, latent k of the shard at a + k lda): sgn * (-d value / d r_l), so sgn = 1 for alpha = -d lml / d r (exact, state space)
  // and -1 for d elbo / d r itself; negation is exact, so one sign serves them bit for bit.  dot (device, n per latent): what
  // aTy_k = a_k . dot_k is taken with, T y of all m latents (dot_all: ONE ms x m launch, [k, l0 + k] read) or a row per latent of the
  // shard (a launch each; atb_kernel computes each output element in a block of its own, so its bits do not depend on the launch).
  const double* a = nullptr; int lda = 0; double sgn = 1.0; const double* dot = nullptr; bool dot_all = false;
  bool want_sum = false;      // asum[k] = sum_t a_t too, for a path with no other source of the mean's gradient (the inducing-point one)
};
// The constructor queues the products on streams[0] with their read-backs: YA = Y'a (p x ms), aTy and, with the regulariser,
// M2 = Y Y' (p x p) per noise block.  finish() is host work for once streams[0] has drained.
struct OilmmGradBackEnd : OilmmGradIn {
  const int ms, mk;
  Buf<double> YAd, aTyd, M2d, ones, asumd;
  std::vector<double> YA, aTy, M2all, asum;
  explicit OilmmGradBackEnd(const OilmmGradIn& in)
      : OilmmGradIn(in), ms(l1 - l0), mk(std::max(ms, 1)), YAd((size_t)p * mk), aTyd((size_t)mk * (dot_all ? m : 1)), M2d((size_t)p * p * NB.nblk),
        YA(YAd.n, 0.0), aTy(aTyd.n, 0.0), M2all(M2d.n, 0.0), asum(mk, 0.0) {
    hipStream_t st0 = g.streams[0];
    if (ms > 0) {
      if (want_sum) { ones = Buf<double>(n); asumd = Buf<double>(mk); launch_fill(ones.p, n, 1.0, st0); }
      launch_atb(yd, n, a, lda, n, p, ms, YAd.p, st0);
      if (want_sum) launch_atb(a, lda, ones.p, n, n, ms, 1, asumd.p, st0);
      if (dot_all) launch_atb(a, lda, dot, n, n, ms, m, aTyd.p, st0);
      else for (int k = 0; k < ms; ++k) launch_atb(a + (size_t)k * lda, lda, dot + (size_t)k * n, n, n, 1, 1, aTyd.p + k, st0);
      HIPCHK(hipMemcpyAsync(YA.data(), YAd.p, YA.size() * sizeof(double), hipMemcpyDeviceToHost, st0));
      HIPCHK(hipMemcpyAsync(aTy.data(), aTyd.p, aTy.size() * sizeof(double), hipMemcpyDeviceToHost, st0));
      if (want_sum) HIPCHK(hipMemcpyAsync(asum.data(), asumd.p, (size_t)ms * sizeof(double), hipMemcpyDeviceToHost, st0));
    }
    if (with_regulariser) {
      for (int b = 0; b < NB.nblk; ++b) launch_atb(yd + NB.off[b], n, yd + NB.off[b], n, NB.count(b), p, p, M2d.p + (size_t)p * p * b, st0);
      HIPCHK(hipMemcpyAsync(M2all.data(), M2d.p, M2all.size() * sizeof(double), hipMemcpyDeviceToHost, st0));
    }
  }
  // dnoise[k * nblk + b]: d value / d (projected noise of latent k of the shard in block b); dot_add[k] (or nullptr): what aTy_k lacks
  // (the state-space path dots with r, the mean taken off: mean_l * sum_t a_t); T: m x p.  Adds the shard's share to G.gs2 / gS / gU,
  // then the regulariser's to them and its value to `value`, and writes gy_dev (n x p, device) when given.
  void finish(const double* dnoise, const double* dot_add, const std::vector<double>& T, double& value, OilmmGrad& G, double* gy_dev) const {
    hipStream_t st0 = g.streams[0];
    const int nblk = NB.nblk;
    for (int k = 0; k < ms; ++k) {
      const int l = l0 + k;
      double g_s2 = 0.0;                                   // sum_b s2[b] d value / d noise_b
      for (int b = 0; b < nblk; ++b) {
        const double gb = dnoise[(size_t)k * nblk + b];
        G.gs2[b] += gb / S[l];
        g_s2 += gb * NB.s2[b];
      }
      double aTyl = dot_all ? aTy[k + (size_t)l * ms] : aTy[k];
      if (dot_add) aTyl += dot_add[k];
      G.gS[l] += -g_s2 / (S[l] * S[l]) + 0.5 * (sgn * aTyl) / S[l];
      for (int o = 0; o < p; ++o) G.gU[o + (size_t)l * p] += -(sgn * YA[o + (size_t)k * p]) / std::sqrt(S[l]);
    }
    std::vector<double> PtP;       // P'P for the regulariser's dY
    if (with_regulariser) oilmm_regulariser_grad(U, S, p, m, NB, M2all, value, G, PtP);
    if (!gy_dev) return;
    // d value / dY[o, i] = -sgn sum_l T[l, o] a_l[i] - (P'P Y)[o, i] / sigma2(i)
    std::vector<double> Tt((size_t)p * mk, 0.0);
    for (int k = 0; k < ms; ++k) for (int o = 0; o < p; ++o) Tt[o + (size_t)k * p] = -(sgn * T[(l0 + k) + (size_t)o * m]);
    Uploaded Ttd(Tt, st0);
    Buf<double> ga((size_t)n * p), ac;
    const double* lat = a;
    if (lda != n) {      // mix reads lat[l * n + i]: a compact copy first
      ac = Buf<double>((size_t)n * mk);
      for (int k = 0; k < ms; ++k) HIPCHK(hipMemcpyAsync(ac.p + (size_t)k * n, a + (size_t)k * lda, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st0));
      lat = ac.p;
    }
    launch_mix(lat, n, ms, Ttd.buf.p, p, 1, 0.0, 0.0, nullptr, 0.0, with_regulariser ? ga.p : gy_dev, st0);
    Uploaded Qd;
    Buf<double> gq;
    if (with_regulariser) {
      Qd = Uploaded(PtP, st0);
      gq = Buf<double>((size_t)n * p);
      launch_tall_skinny(yd, n, n, p, Qd.buf.p, p, p, gq.p, n, nullptr, nullptr, 0, nullptr, 0, st0);   // (Y' (P'P)')' rows
      launch_vec_lin_blocks(ga.p, gq.p, NB, -1.0, n, (size_t)n * p, gy_dev, st0);
    }
    HIPCHK(hipStreamSynchronize(st0));         // Ttd, ga, ac, gq and Qd are released on return
  }
};

// What oilmm_grad_core and oilmm_grad_missing_core share, per latent of the shard: the training matrix with the residual as its rider,
// its factor, alpha = Kt^-1 delta, Kt^-1 = L^-T L^-1 (triangular solve of identity riders + an upper-triangular SYRK, over the factor's
// lower triangle) and one kernel-gradient reduction per term; then the read-back of the reductions and the host formulas of the
// latent's own (variance, lengthscale, mean) gradients.  What a caller does with the reductions beyond that stays with the caller.
struct KernelGradPass {
  const Latent* lts;
  const int l0, ms, n, d, ard_d;
  const Dims D;
  FanOut F;
  std::vector<Slot> slots;
  const std::vector<int> toff;     // one reduction per term of every latent of the shard
  const int nterm;
  Buf<double> alpha, lmld, red, ardred;      // ardred: per-dimension sums of the ARD terms (d/d l_k)
  std::vector<double> lml, hred, hard;       // their host copies (read_back)

  KernelGradPass(const LatentSet* ls, int l0_, int l1, int n_, int d_)
      : lts(ls->lat.data()), l0(l0_), ms(l1 - l0_), n(n_), d(d_), ard_d(ls->ard_grad_d()), D(n_, 1),
        F(ms, 2.0 * mat_bytes((double)D.elems())),     // factor + inverse-factor matrices
        toff(ls->term_offsets(l0_, l1)), nterm(toff[ms]),
        alpha((size_t)D.NC * F.mk), lmld(F.mk), red((size_t)LMM_NGRAD * std::max(nterm, 1)), ardred((size_t)d * std::max(nterm, 1)) {
    make_slots(slots, F.nslots, F.nb_per, D.elems(), D.NC, (size_t)D.ld * D.NC, (size_t)grad_partials(n, ard_d));
    F.alloc_info();
    HIPCHK(hipMemsetAsync(alpha.p, 0, (size_t)D.NC * F.mk * sizeof(double), g.streams[0]));
  }

  // delta: the residuals ([latent of the shard][n], device); the noise: noise[latent] (host), or per point noisevec ([latent of the
  // shard][n], device) when given; nsplit: where the contraction kernel splits its trace / alpha.alpha sums.  The hooks run on the
  // batch's stream with Kt^-1 and alpha of latent k (shard index): per_term after the reduction of each of its terms (gd),
  // per_latent after the last.
  template <class PerTerm, class PerLatent>
  void launch(const double* xd, const double* delta, const double* noise, const double* noisevec, int nsplit, PerTerm&& per_term,
              PerLatent&& per_latent) {
    F.run([&](const FanBatch& b) {
      Slot& s = slots[b.s];
      hipStream_t st = b.st;
      const int nb = b.nb;
      Batch B;
      BatchPtr Rb{}, alb{};
      GramArgs ga[LMM_MAX_BATCH];
      for (int j = 0; j < nb; ++j) {
        const int k = b.k0 + j;
        ga[j] = train_gram_args(lts[l0 + k], xd, d, n, D, s.A[j].p, noisevec ? 0.0 : noise[l0 + k],
                                noisevec ? noisevec + (size_t)k * n : nullptr, delta + (size_t)k * n, 1);
        B.add(s.A[j].p, s.W[j].p, F.info + k);
        Rb.p[j] = s.R[j].p; alb.p[j] = alpha.p + (size_t)k * D.NC;
      }
      gram_batch_g(ga, nb, st);
      potrf_batch(B, D.ld, D.NR, D.NC, n, st, D.NC + 1);        // one rider row (delta); rows NC + 1 .. NR - 1 are zero padding
      launch_lml_reduce(B.A, nb, D.ld, n, D.NC, 1, lmld.p + b.k0, st);
      for (int j = 0; j < nb; ++j) {
        launch_extract_row(s.A[j].p, D.ld, D.NC, n, alb.p[j], st);
        launch_set_identity(s.R[j].p, D.ld, D.NC, st);
      }
      launch_backsolve(B.A, D.ld, B.W, D.NC / 64, alb, nb, st);
      trsm_rec(Rb, D.ld, D.NC, B.A, D.ld, B.W, nb, 0, D.NC, st, true);        // R = L^-T (upper triangular), whole batch
      launch_syrk_upper_set(B.A, D.ld, Rb, D.ld, D.NC, nb, st);                // lower(A) = L^-T L^-1 = Kt^-1
      for (int j = 0; j < nb; ++j) {
        const int k = b.k0 + j;
        // one reduction per term (the trace and alpha.delta partials, which do not depend on the kernel, are read from term 0's)
        for (int c = 0; c < lts[l0 + k].nt(); ++c) {
          const LatentDev& gd = lts[l0 + k].terms[c].gd;
          const size_t t = (size_t)toff[k] + c;
          launch_grad_reduce(s.A[j].p, D.ld, n, nsplit, alb.p[j], delta + (size_t)k * n, xd, d, gd, s.part.p, red.p + LMM_NGRAD * t, st,
                             ardred.p + d * t);
          per_term(b, k, s.A[j].p, alb.p[j], gd);
        }
        per_latent(b, k, s.A[j].p, alb.p[j]);
      }
    });
  }

  void read_back() {       // queued on the main stream after the join: lml, the reductions and the ARD sums
    hipStream_t st0 = g.streams[0];
    lml.assign(F.mk, 0.0); hred.assign((size_t)LMM_NGRAD * std::max(nterm, 1), 0.0);
    HIPCHK(hipMemcpyAsync(lml.data(), lmld.p, F.mk * sizeof(double), hipMemcpyDeviceToHost, st0));
    HIPCHK(hipMemcpyAsync(hred.data(), red.p, hred.size() * sizeof(double), hipMemcpyDeviceToHost, st0));
    hard.assign(ard_d ? (size_t)d * std::max(nterm, 1) : 0, 0.0);
    if (!hard.empty()) HIPCHK(hipMemcpyAsync(hard.data(), ardred.p, hard.size() * sizeof(double), hipMemcpyDeviceToHost, st0));
  }

  // ---- host, once the main stream has drained ----
  // the sums of latent k's first term: [1] tr Kt^-1 and [2] alpha.alpha over the rows below nsplit ([5], [6]: from nsplit on),
  // [3] alpha.delta, [4] sum(alpha)
  const double* sums(int k) const { return &hred[(size_t)LMM_NGRAD * toff[k]]; }
  // ggps[l] and the term records of latent k from D_aa = alpha' D alpha and D_tr = tr(Kt^-1 D), D its diagonal noise, and
  // alpha.alpha, tr Kt^-1 over all rows
  void finish(int k, double D_aa, double D_tr, double aa, double tr, std::vector<lmm_gp_grad_t>& ggps, std::vector<double>& trec) const {
    const int l = l0 + k;
    const double* r = sums(k);
    // 1/2 tr((aa' - Kt^-1) K) / v  with K = Kt - D:  a'delta - a'Da - (n - tr(Kt^-1 D))     (a sum latent's K is linear in v0 too)
    ggps[l].variance = 0.5 * ((r[3] - D_aa) - ((double)n - D_tr)) / lts[l].variance;
    // sum_{i>j} (a_i a_j - Kinv_ij) dK_ij/dl (x2 / 2), through the terms
    ggps[l].lengthscale = grad_finish(lts[l], d, r, hard.empty() ? nullptr : &hard[(size_t)d * toff[k]], aa, tr,
                                      &trec[(size_t)l * LMM_SUM_MAX_TERMS * term_grad_stride(d)]);
    ggps[l].mean = r[4];
  }
};

// Sum of the per-slot accumulators into out, in slot order (so the result does not depend on stream timing), skipping slots that
// carried no latent; on the main stream after the join.  Returns false when no slot was used (out untouched).  axpby: the caller's
// add is vec_axpby_kernel, else vec_lin_kernel -- out + 1.0 * acc and 1.0 * out + 1.0 * acc round alike, but each caller keeps its launch.
bool sum_slots(double* out, const std::vector<Buf<double>>& acc, const std::vector<char>& used, size_t count, hipStream_t st0,
               bool axpby = false) {
  bool first = true;
  for (size_t s = 0; s < acc.size(); ++s) {
    if (!used[s]) continue;
    if (first) HIPCHK(hipMemcpyAsync(out, acc[s].p, count * sizeof(double), hipMemcpyDeviceToDevice, st0));
    else if (axpby) launch_vec_axpby(out, 1.0, acc[s].p, 1.0, count, out, st0);
    else launch_vec_lin(out, acc[s].p, 1.0, (int)count, out, st0);
    first = false;
  }
  return !first;
}

// Value and gradient of the OILMM logpdf (reference src/oilmm.jl:79-113 differentiated) over N points in NB.nblk consecutive
// blocks, block b carrying observation noise NB.s2[b] (one block: the plain logpdf; several: the joint density of the
// conditioning batches and the test points that the predictive logpdf is the difference of).  Per latent: factor, alpha = Kt^-1 delta, Kt^-1 = L^-T L^-1
// (triangular solve of identity riders + an upper-triangular SYRK on the MFMA kernels), one fused contraction kernel; the chain
// rule through T = S^-1/2 U', the projected noise s2/S and the regulariser is small host algebra.
// xd: d x N (device), yd: N x p column-major (device), gy_dev: N x p device output or nullptr.  gx_dev: d x N device output of
// d logpdf / d x summed over the shard's latents (grad_x_kernel), or nullptr (no launch, no allocation).  Caller holds g_mu.
int oilmm_grad_core(const double* xd, int d, int N, const NoiseBlocks& NB, const double* yd, int p, const double* U, const double* S,
                    const LatentSet* ls, int l0, int l1, int with_regulariser, OilmmGrad& G, double* gy_dev,
                    double* gx_dev = nullptr) {
  hipStream_t st0 = g.streams[0];
  const int m = (int)ls->lat.size();
  const Latent* lts = ls->lat.data();
  const int ms = l1 - l0, mk = std::max(ms, 1), n = N, nblk = NB.nblk;      // mk: what the per-latent buffers of a possibly empty shard take
  const bool two = nblk > 1;
  const int nsplit = nblk == 2 ? NB.off[1] : N;        // the contraction kernel splits its trace / alpha.alpha sums once
  std::vector<double> T, STa, H;
  project_orthogonal(U, S, p, m, NB.s2[0], T, STa, H);
  std::vector<std::vector<double>> ST(nblk, std::vector<double>(m));      // projected noise s2[b] / S[l]
  for (int b = 0; b < nblk; ++b)
    for (int l = 0; l < m; ++l) ST[b][l] = NB.s2[b] / S[l];
  const std::vector<double> means = latent_means(lts, m);
  Uploaded Td(T, st0), meansd(means, st0);
  // projections: Ty (all m, for dS), delta for the shard
  Buf<double> Ty((size_t)n * m), delta((size_t)n * mk);
  project_on_device(yd, n, p, Td.buf, m, 0, m, nullptr, Ty.p, st0);
  if (ms > 0) project_on_device(yd, n, p, Td.buf, m, l0, ms, meansd.buf.p + l0, delta.p, st0);
  Buf<double> nv(two ? (size_t)n * mk : 1);          // per-point projected noise of the shard's latents
  if (two)
    for (int k = 0; k < ms; ++k)
      for (int b = 0; b < nblk; ++b) launch_fill(nv.p + (size_t)k * n + NB.off[b], NB.count(b), ST[b][l0 + k], st0);
  KernelGradPass K(ls, l0, l1, n, d);
  const Dims& D = K.D;
  const int nslots = K.F.nslots;
  Buf<double>& alpha = K.alpha;
  // more than two noise blocks: [tr Kinv, alpha.alpha] per (latent, block) from the small per-range kernels
  Buf<double> blksum(nblk > 2 ? (size_t)2 * nblk * mk : 1);
  // input gradient: each slot sums its latents (in order) into its own d x N buffer; the slots are summed in slot order after the join
  std::vector<Buf<double>> gxpart, gxacc;
  std::vector<char> gx_used(nslots, 0);
  if (gx_dev)
    for (int s = 0; s < nslots; ++s) { gxpart.emplace_back(grad_x_partial_elems(n, d)); gxacc.emplace_back((size_t)d * n); }
  K.launch(xd, delta.p, two ? nullptr : STa.data(), two ? nv.p : nullptr, nsplit,
           [&](const FanBatch& b, int, const double* Kinv, const double* al, const LatentDev& gd) {
             if (!gx_dev) return;
             launch_grad_x(Kinv, D.ld, n, al, xd, d, gd, gxpart[b.s].p, gxacc[b.s].p, gx_used[b.s] != 0, b.st);
             gx_used[b.s] = 1;
           },
           [&](const FanBatch& b, int k, const double* Kinv, const double* al) {
             if (nblk > 2)
               for (int blk = 0; blk < nblk; ++blk) {
                 double* o = blksum.p + ((size_t)k * nblk + blk) * 2;
                 launch_block_trace(Kinv, D.ld, n, 1, NB.off[blk], NB.off[blk + 1], o, b.st);
                 launch_atb(al + NB.off[blk], n, al + NB.off[blk], n, NB.count(blk), 1, 1, o + 1, b.st);
               }
           });
  if (gx_dev && !sum_slots(gx_dev, gxacc, gx_used, (size_t)d * n, st0))
    HIPCHK(hipMemsetAsync(gx_dev, 0, (size_t)d * n * sizeof(double), st0));      // empty shard
  K.read_back();
  std::vector<double> hblk(nblk > 2 ? (size_t)2 * nblk * mk : 0, 0.0);
  if (!hblk.empty() && ms > 0) HIPCHK(hipMemcpyAsync(hblk.data(), blksum.p, hblk.size() * sizeof(double), hipMemcpyDeviceToHost, st0));
  K.F.fetch_info();
  // the back end's products are queued ahead of the wait for the pivots; alpha = -d lml / d delta, dotted with T y itself
  OilmmGradIn in{yd, n, p, U, S, m, NB, l0, l1, with_regulariser};
  in.a = alpha.p; in.lda = D.NC; in.dot = Ty.p; in.dot_all = true;
  OilmmGradBackEnd B(in);
  if (int rc = K.F.check(l0)) return rc;

  // ---- host: the latents' own gradients and d lml / d (projected noise) per block ----
  double total = 0.0;
  G.size(m, p, nblk, d);
  std::vector<double> dnoise((size_t)mk * nblk, 0.0);
  for (int k = 0; k < ms; ++k) {
    const int l = l0 + k;
    total += K.lml[k];
    const double* r = K.sums(k);
    double aa_all = 0.0, tr_all = 0.0;
    double D_aa = 0.0, D_tr = 0.0;       // a'Da, tr(Kt^-1 D) with D the projected noise
    for (int b = 0; b < nblk; ++b) {
      // tr Kinv and alpha.alpha over the block's rows
      const double tr = nblk > 2 ? hblk[((size_t)k * nblk + b) * 2] : r[b ? 5 : 1];
      const double aa = nblk > 2 ? hblk[((size_t)k * nblk + b) * 2 + 1] : r[b ? 6 : 2];
      dnoise[(size_t)k * nblk + b] = 0.5 * (aa - tr);
      D_aa += ST[b][l] * aa; D_tr += ST[b][l] * tr;
      aa_all += aa; tr_all += tr;
    }
    K.finish(k, D_aa, D_tr, aa_all, tr_all, G.ggps, G.trec);
  }
  B.finish(dnoise.data(), nullptr, T, total, G, gy_dev);
  G.value = total;
  return LMM_OK;
}

// Predictive input gradients from the joint (d x (n + ns), device) and marginal (d x n, device) ones: grad_x = joint[:, :n] - marginal,
// grad_xs = joint[:, n:].  Either output may be NULL (host or device pointers).
int finish_input_grads(const double* gxj, const double* gxm, int d, int n, int ns, double* grad_x, double* grad_xs) {
  hipStream_t st0 = g.streams[0];
  if (grad_x) {
    DevOut o(grad_x, (size_t)d * n);
    launch_vec_lin(gxj, gxm, -1.0, d * n, o.p, st0);
    o.finish(st0);
    HIPCHK(hipStreamSynchronize(st0));
  }
  if (grad_xs) {
    DevOut o(grad_xs, (size_t)d * ns);
    HIPCHK(hipMemcpyAsync(o.p, gxj + (size_t)d * n, (size_t)d * ns * sizeof(double), hipMemcpyDeviceToDevice, st0));
    o.finish(st0);
    HIPCHK(hipStreamSynchronize(st0));
  }
  return LMM_OK;
}

// The driver of the predictive gradients, log p(ys | y) = log p(y, ys) - log p(y): `core(joint, x, n, NB, y, G, gy, gx)` is the model's
// prior-gradient core (oilmm_grad_core, ilmm_grad_core), run on the joint [x; xs], [y; ys] with one noise block per conditioning batch
// and one for the test points, then on the conditioning data alone.  xd (d x n), yd (n x p by outputs): device; xs, ys: the caller's.  ys
// has pt <= p columns (the dense-H latent view observes m of the p outputs): the joint's other test columns are zero.  Leaves the two
// results in GJ and GM for the model's own outputs, with GJ.ggps and GJ.trec already the differences (published, and written to
// grad_gps), and writes every output the models share: grad_y, grad_ys (ns x pt), grad_batch_sigma2, grad_x, grad_xs.
template <class Grad, class Core>
int predictive_grad(const LatentSet& ls, int l0, int l1, const double* xd, const double* yd, int d, int n, const int* batch_n,
                    const double* batch_sigma2, int nbatch, const double* xs, int ns, const double* ys, int p, int pt, double sigma2_s,
                    Core core, Grad& GJ, Grad& GM, double* grad_y, double* grad_ys, double* grad_batch_sigma2, lmm_gp_grad_t* grad_gps,
                    double* grad_x, double* grad_xs) {
  hipStream_t st0 = g.streams[0];
  const int N = n + ns;
  const size_t col = sizeof(double);
  DevIn xsd(xs, (size_t)d * ns, st0), ysd(ys, (size_t)ns * pt, st0);
  Buf<double> xj((size_t)d * N), yj((size_t)N * p), gj((size_t)N * p), gm((size_t)n * p);
  HIPCHK(hipMemcpyAsync(xj.p, xd, (size_t)d * n * col, hipMemcpyDeviceToDevice, st0));
  HIPCHK(hipMemcpyAsync(xj.p + (size_t)d * n, xsd.p, (size_t)d * ns * col, hipMemcpyDeviceToDevice, st0));
  if (pt < p) HIPCHK(hipMemsetAsync(yj.p, 0, (size_t)N * p * col, st0));
  HIPCHK(hipMemcpy2DAsync(yj.p, N * col, yd, n * col, n * col, p, hipMemcpyDeviceToDevice, st0));
  HIPCHK(hipMemcpy2DAsync(yj.p + n, N * col, ysd.p, ns * col, ns * col, pt, hipMemcpyDeviceToDevice, st0));
  if (int rc = ls.ard_grad_check()) return rc;
  const bool want_gx = grad_x != nullptr || grad_xs != nullptr, want_gy = grad_y != nullptr || grad_ys != nullptr;
  if (int rc = input_grad_check(d, want_gx)) return rc;
  if (want_gx) { if (int rc = refuse_sho(ls, "gradients with respect to the inputs are")) return rc; }
  Buf<double> gxj, gxm;
  if (want_gx) gxj = Buf<double>((size_t)d * N);
  if (grad_x) gxm = Buf<double>((size_t)d * n);
  if (int rc = core(true, xj.p, N, batch_noise_blocks(batch_n, batch_sigma2, nbatch, ns, sigma2_s), yj.p, GJ, want_gy ? gj.p : nullptr, gxj.p)) return rc;
  if (int rc = core(false, xd, n, batch_noise_blocks(batch_n, batch_sigma2, nbatch, 0, 0.0), yd, GM, grad_y ? gm.p : nullptr, gxm.p)) return rc;
  if (int rc = finish_input_grads(gxj.p, gxm.p, d, n, ns, grad_x, grad_xs)) return rc;
  if (grad_batch_sigma2) for (int b = 0; b < nbatch; ++b) grad_batch_sigma2[b] = GJ.gs2[b] - GM.gs2[b];
  for (size_t l = 0; l < GJ.ggps.size(); ++l) {
    GJ.ggps[l].variance -= GM.ggps[l].variance;
    GJ.ggps[l].lengthscale -= GM.ggps[l].lengthscale;
    GJ.ggps[l].mean -= GM.ggps[l].mean;
  }
  for (size_t q = 0; q < GJ.trec.size(); ++q) GJ.trec[q] -= GM.trec[q];
  publish_grads(ls, grad_gps ? &GJ.trec : nullptr, l0, l1);
  if (grad_gps) std::copy(GJ.ggps.begin(), GJ.ggps.end(), grad_gps);
  if (grad_y) {
    DevOut gy(grad_y, (size_t)n * p);
    Buf<double> top((size_t)n * p);
    HIPCHK(hipMemcpy2DAsync(top.p, n * col, gj.p, N * col, n * col, p, hipMemcpyDeviceToDevice, st0));
    launch_vec_lin(top.p, gm.p, -1.0, n * p, gy.p, st0);
    gy.finish(st0);
    HIPCHK(hipStreamSynchronize(st0));
  }
  if (grad_ys) {
    DevOut gys(grad_ys, (size_t)ns * pt);
    HIPCHK(hipMemcpy2DAsync(gys.p, ns * col, gj.p + n, N * col, ns * col, pt, hipMemcpyDeviceToDevice, st0));
    gys.finish(st0);
    HIPCHK(hipStreamSynchronize(st0));
  }
  return LMM_OK;
}

void write_oilmm_grad(const OilmmGrad& G, double* out_value, double* grad_sigma2, double* grad_S, double* grad_U, lmm_gp_grad_t* grad_gps) {
  if (out_value) *out_value = G.value;
  if (grad_sigma2) { *grad_sigma2 = 0.0; for (double v : G.gs2) *grad_sigma2 += v; }
  if (grad_S) std::copy(G.gS.begin(), G.gS.end(), grad_S);
  if (grad_U) std::copy(G.gU.begin(), G.gU.end(), grad_U);
  if (grad_gps) std::copy(G.ggps.begin(), G.ggps.end(), grad_gps);
}

}  // namespace

extern "C" {

// Value and gradient of logpdf(fx::FiniteGP{<:OILMM}, y) (reference src/oilmm.jl:79-93; what the reference's
// Zygote.gradient(logpdf, fx, y) differentiates, test/oilmm.jl:31-32) w.r.t. y, sigma2, S, U and every latent's
// (variance, lengthscale, mean).  Partial sums over the shard.
int lmm_oilmm_logpdf_grad_x(const double* x, int d, int n, const double* y, int p, const double* U, const double* S, int m,
                            double sigma2, const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser,
                            double* out_logpdf, double* grad_y, double* grad_sigma2, double* grad_S, double* grad_U,
                            lmm_gp_grad_t* grad_gps, double* grad_x) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  // fp32 compute mode (round 3): Float32 factor, triangular inverse and K^-1 = L^-T L^-1 (all on v_mfma_f32), Float64 reductions;
  // stated tolerance against the Float64 gradient: include/lmm_hip.h
  Train R;
  if (int rc = train(!x || !y || !U || !S || !out_logpdf || d <= 0 || n <= 0 || p <= 0 || m <= 0, x, d, n, y, (size_t)n * p, p, S, m, sigma2, gps,
                     latent_begin, latent_end, 0, R)) return rc;
  if (!(sigma2 > 0.0)) return fail(LMM_ERR_ARG, "sigma2 must be > 0");
  hipStream_t st0 = g.streams[0];
  DevOut gy(grad_y, (size_t)n * p), gx(grad_x, (size_t)d * n);
  if (int rc = R.ls->ard_grad_check()) return rc;
  if (int rc = input_grad_check(d, grad_x != nullptr)) return rc;
  if (grad_x) { if (int rc = refuse_sho(*R.ls, "gradients with respect to the inputs are")) return rc; }
  OilmmGrad G;
  if (int rc = oilmm_grad_core(R.xd.p, d, n, one_noise_block(n, sigma2), R.yd.p, p, U, S, R.ls.get(), latent_begin, latent_end, with_regulariser,
                               G, gy.p, gx.p))
    return rc;
  write_oilmm_grad(G, out_logpdf, grad_sigma2, grad_S, grad_U, grad_gps);
  publish_grads(*R.ls, grad_gps ? &G.trec : nullptr, latent_begin, latent_end);
  if (grad_y) gy.finish(st0);
  if (grad_x) gx.finish(st0);
  if (grad_y || grad_x) HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

int lmm_oilmm_logpdf_grad(const double* x, int d, int n, const double* y, int p, const double* U, const double* S, int m,
                          double sigma2, const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser,
                          double* out_logpdf, double* grad_y, double* grad_sigma2, double* grad_S, double* grad_U,
                          lmm_gp_grad_t* grad_gps) {
  return lmm_oilmm_logpdf_grad_x(x, d, n, y, p, U, S, m, sigma2, gps, latent_begin, latent_end, with_regulariser, out_logpdf, grad_y,
                                 grad_sigma2, grad_S, grad_U, grad_gps, nullptr);
}

// Value and gradient of the predictive logpdf  logpdf(posterior(f(x, sigma2), y)(xs, sigma2_s), ys)  of an OILMM (or, with
// U = I, S = 1, an IndependentMOGP) -- the reference takes Zygote.gradient(logpdf, po_x, y*) on the posterior models
// (test/oilmm.jl:32, test/independent_mogp.jl:66).  Exact conditioning gives, latent by latent and for the regulariser,
//     log p(ys | y) = log p(y, ys) - log p(y),
// so value and TOTAL derivatives (through alpha, the factor and the Schur complement of the posterior) are the difference of
// two evaluations of the prior-logpdf gradient: the joint over [x; xs] with per-block noise, and the marginal over x.
// _seq: the posterior was conditioned SEQUENTIALLY, posterior(posterior(f(x1, s1), y1)(x2, s2), y2) ... (reference
// src/oilmm.jl:116-134 applied to its own result); exact conditioning makes that the posterior given all batches at once with
// per-batch noise.  x (d x n) and y (n x p by outputs) hold the batches' points in conditioning order, n = sum batch_n.
int lmm_oilmm_post_logpdf_grad_seq_x(const double* x, int d, int n, const int* batch_n, const double* batch_sigma2, int nbatch,
                                     const double* y, const double* xs, int ns, const double* ys, int p, const double* U,
                                     const double* S, int m, double sigma2_s, const lmm_gp_t* gps, int latent_begin, int latent_end,
                                     int with_regulariser, double* out_logpdf, double* grad_y, double* grad_ys,
                                     double* grad_batch_sigma2, double* grad_sigma2_s, double* grad_S, double* grad_U,
                                     lmm_gp_grad_t* grad_gps, double* grad_x, double* grad_xs) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  // (the same core with one noise block per conditioning batch + one for the test points: served in the fp32 compute mode too)
  Train R;
  if (int rc = train(!x || !y || !xs || !ys || !U || !S || !out_logpdf || d <= 0 || n <= 0 || ns <= 0 || p <= 0 || m <= 0, x, d, n, y, (size_t)n * p, p,
                     S, m, sigma2_s, gps, latent_begin, latent_end, 0, R)) return rc;
  if (int rc = check_batches(batch_n, batch_sigma2, nbatch, n)) return rc;
  if (!(sigma2_s > 0.0)) return fail(LMM_ERR_ARG, "sigma2 must be > 0");
  OilmmGrad GJ, GM;
  auto core = [&](bool, const double* xq, int nq, const NoiseBlocks& NB, const double* yq, OilmmGrad& G, double* gy, double* gx) {
    return oilmm_grad_core(xq, d, nq, NB, yq, p, U, S, R.ls.get(), latent_begin, latent_end, with_regulariser, G, gy, gx);
  };
  if (int rc = predictive_grad(*R.ls, latent_begin, latent_end, R.xd.p, R.yd.p, d, n, batch_n, batch_sigma2, nbatch, xs, ns, ys, p, p, sigma2_s,
                               core, GJ, GM, grad_y, grad_ys, grad_batch_sigma2, grad_gps, grad_x, grad_xs)) return rc;
  *out_logpdf = GJ.value - GM.value;
  if (grad_sigma2_s) *grad_sigma2_s = GJ.gs2[nbatch];
  if (grad_S) for (int l = 0; l < m; ++l) grad_S[l] = GJ.gS[l] - GM.gS[l];
  if (grad_U) for (size_t q = 0; q < (size_t)p * m; ++q) grad_U[q] = GJ.gU[q] - GM.gU[q];
  return LMM_OK;
  LMM_CATCH
}

int lmm_oilmm_post_logpdf_grad_seq(const double* x, int d, int n, const int* batch_n, const double* batch_sigma2, int nbatch,
                                   const double* y, const double* xs, int ns, const double* ys, int p, const double* U,
                                   const double* S, int m, double sigma2_s, const lmm_gp_t* gps, int latent_begin, int latent_end,
                                   int with_regulariser, double* out_logpdf, double* grad_y, double* grad_ys,
                                   double* grad_batch_sigma2, double* grad_sigma2_s, double* grad_S, double* grad_U,
                                   lmm_gp_grad_t* grad_gps) {
  return lmm_oilmm_post_logpdf_grad_seq_x(x, d, n, batch_n, batch_sigma2, nbatch, y, xs, ns, ys, p, U, S, m, sigma2_s, gps, latent_begin,
                                          latent_end, with_regulariser, out_logpdf, grad_y, grad_ys, grad_batch_sigma2, grad_sigma2_s,
                                          grad_S, grad_U, grad_gps, nullptr, nullptr);
}

// One conditioning batch: posterior(f(x, sigma2), y).
int lmm_oilmm_post_logpdf_grad(const double* x, int d, int n, const double* y, const double* xs, int ns, const double* ys, int p,
                               const double* U, const double* S, int m, double sigma2, double sigma2_s, const lmm_gp_t* gps,
                               int latent_begin, int latent_end, int with_regulariser, double* out_logpdf, double* grad_y,
                               double* grad_ys, double* grad_sigma2, double* grad_sigma2_s, double* grad_S, double* grad_U,
                               lmm_gp_grad_t* grad_gps) {
  return lmm_oilmm_post_logpdf_grad_seq(x, d, n, &n, &sigma2, 1, y, xs, ns, ys, p, U, S, m, sigma2_s, gps, latent_begin, latent_end,
                                        with_regulariser, out_logpdf, grad_y, grad_ys, grad_sigma2, grad_sigma2_s, grad_S, grad_U, grad_gps);
}

// logpdf(fx, Y::AbstractMatrix) -- one logpdf per column of Y with ONE factorisation per latent (SURVEY.md 8f next #3;
// the reference answers it through AbstractGPs' dense generic fallback).  Y is (n p) x ncol column-major.
int lmm_oilmm_logpdf_multi(const double* x, int d, int n, const double* Y, int p, int ncol, const double* U, const double* S,
                           int m, double sigma2, const lmm_gp_t* gps, int latent_begin, int latent_end,
                           int with_regulariser, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  Train R;
  if (int rc = train(!x || !Y || !U || !S || !out || d <= 0 || n <= 0 || p <= 0 || m <= 0 || ncol <= 0, x, d, n, Y, (size_t)n * p * ncol, p, S, m, sigma2,
                     gps, latent_begin, latent_end, 0, R)) return rc;
  hipStream_t st0 = g.streams[0];
  OilmmFront F(U, S, p, m, sigma2);
  F.upload(R.means);
  Uploaded Hd(F.H, st0);
  const int l0 = R.l0, l1 = R.l1, ms = R.ms;
  Buf<double> delta((size_t)n * R.mk * ncol), Ty((size_t)n * m), partial(tall_skinny_partials(n, p)), resid_dev(ncol);
  std::vector<double> resid(ncol, 0.0);
  for (int c = 0; c < ncol; ++c) {
    const double* yc = R.yd.p + (size_t)c * n * p;
    // rider [latent k][column c]: delta + (k ncol + c) n  ==  output column stride ncol*n
    if (ms > 0) launch_tall_skinny(yc, n, n, p, F.Td.buf.p + l0, m, ms, delta.p + (size_t)c * n, ncol * n, F.meansd.buf.p + l0, nullptr, 0,
                                   nullptr, 0, st0);
    if (with_regulariser) {
      project_on_device(yc, n, p, F.Td.buf, m, 0, m, nullptr, Ty.p, st0);
      residual_on_device(yc, n, p, Ty.p, m, Hd.buf, partial.p, resid_dev.p + c, st0);
    }
  }
  if (with_regulariser) HIPCHK(hipMemcpyAsync(resid.data(), resid_dev.p, ncol * sizeof(double), hipMemcpyDeviceToHost, st0));
  std::vector<double> lml;
  if (int rc = latent_lmls(R.xd.p, d, n, R.lts, F.ST.data(), l0, l1, delta.p, lml, ncol)) return rc;
  for (int c = 0; c < ncol; ++c) {
    double total = 0.0;
    for (int k = 0; k < ms; ++k) total += lml[(size_t)k * ncol + c];
    if (with_regulariser) total += oilmm_regulariser(n, p, m, S, sigma2, resid[c]);
    out[c] = total;
  }
  return LMM_OK;
  LMM_CATCH
}

// MOInputIsotopicByFeatures <-> MOInputIsotopicByOutputs reordering of a length n*p vector (reference
// src/independent_mogp.jl:135-159): to_outputs != 0: out[o n + i] = in[i p + o]; else the inverse.
int lmm_reorder(const double* in, int n, int p, int to_outputs, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!in || !out || n <= 0 || p <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  hipStream_t st0 = g.streams[0];
  DevIn ind(in, (size_t)n * p, st0);
  DevOut od(out, (size_t)n * p);
  launch_reorder(ind.p, n, p, to_outputs, od.p, st0);
  od.finish(st0);
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

int lmm_mogp_logpdf(const double* x, int d, int n, const double* y, int m, double sigma2, const lmm_gp_t* gps,
                    int latent_begin, int latent_end, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  Train R;
  if (int rc = train(!x || !y || !out || d <= 0 || n <= 0 || m <= 0, x, d, n, y, (size_t)n * m, m, nullptr, m, sigma2, gps, latent_begin, latent_end, 0, R))
    return rc;
  // delta_l = y_l - mean_l  via the projection kernel with T = I restricted to the shard
  OilmmFront F = OilmmFront::identity(m);
  F.upload(R.means);
  Buf<double> delta = F.delta(R.yd.p, n, R.l0, R.ms);
  const std::vector<double> noise(m, sigma2);
  std::vector<double> lml;
  if (int rc = latent_lmls(R.xd.p, d, n, R.lts, noise.data(), R.l0, R.l1, delta.p, lml)) return rc;
  double total = 0.0;
  for (int k = 0; k < R.ms; ++k) total += lml[k];
  *out = total;
  return LMM_OK;
  LMM_CATCH
}

int lmm_mogp_logpdf_diag(const double* x, int d, int n, const double* y, int m, const double* noise_diag, const lmm_gp_t* gps,
                         int latent_begin, int latent_end, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  Train R;
  if (int rc = train(!x || !y || !noise_diag || !out || d <= 0 || n <= 0 || m <= 0, x, d, n, y, (size_t)n * m, m, nullptr, m, 0.0, gps, latent_begin,
                     latent_end, 0, R)) return rc;
  DevIn nd(noise_diag, (size_t)n * m, g.streams[0]);
  OilmmFront F = OilmmFront::identity(m);
  F.upload(R.means);
  Buf<double> delta = F.delta(R.yd.p, n, R.l0, R.ms);
  const std::vector<double> noise(m, 0.0);
  std::vector<double> lml;
  if (int rc = latent_lmls(R.xd.p, d, n, R.lts, noise.data(), R.l0, R.l1, delta.p, lml, 1, nd.p + (size_t)R.l0 * n)) return rc;
  double total = 0.0;
  for (int k = 0; k < R.ms; ++k) total += lml[k];
  *out = total;
  return LMM_OK;
  LMM_CATCH
}

int lmm_ilmm_logpdf_ex(const double* x, int d, int n, const double* y, int p, const double* H, int m, double sigma2,
                       const lmm_gp_t* gps, const lmm_jitters_t* jit, int allow_decoupled, int* path_used, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!x || !y || !H || !out || d <= 0 || n <= 0 || p <= 0 || m <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  RESOLVE(gps, m, d);
  if (!jit) jit = &kDefaultJit;
  if ((long long)m * n > 2000000000LL / 64) return fail(LMM_ERR_UNSUPPORTED, "m*n too large for the dense path");
  hipStream_t st0 = g.streams[0];
  DenseFront F(H, p, m);
  if (int rc = F.project(sigma2, jit->project_jitter, true)) return rc;
  DevIn xd(x, (size_t)d * n, st0), yd(y, (size_t)n * p, st0);
  F.upload(lts, n);
  // the regulariser's residual (reference src/ilmm.jl:171-181), then the rider vec(T Y) - mean
  Buf<double> delta((size_t)n * m), resid_dev(1);
  F.residual(yd.p, n, resid_dev.p);
  bool identical = allow_decoupled != 0;
  for (int l = 1; l < m && identical; ++l)
    identical = lts[l].same_kernel(lts[0]);        // two tags with one alpha: one kernel
  if (path_used) *path_used = identical ? 1 : 0;
  if (identical) {
    // Decoupled shortcut: with one shared latent kernel the covariance is I (x) K + SigmaT (x) I;
    // SigmaT = Q Lam Q' rotates it to blockdiag(K + lam_a I), so the (mn)^3/3 factorisation becomes m independent n^3/3
    // ones on the rotated projections (Q'T) Y - Q' mu.  Same value up to rounding; not the reference's operation count.
    std::vector<double> lam, Q;
    host_jacobi_eig(F.ST, m, lam, Q);
    const std::vector<double> T2 = host_matmul(Q.data(), true, F.T.data(), false, m, m, p);      // Q' T
    std::vector<double> mu2(m, 0.0);
    for (int aI = 0; aI < m; ++aI) {
      for (int b = 0; b < m; ++b) mu2[aI] += Q[b + (size_t)aI * m] * lts[b].mean;
      if (!(lam[aI] > 0.0)) return fail(LMM_ERR_NOT_PD, "PosDefException: SigmaT has a non-positive eigenvalue");
    }
    Uploaded T2d(T2, st0), mu2d(mu2, st0);
    project_on_device(yd.p, n, p, T2d.buf, m, 0, m, mu2d.buf.p, delta.p, st0);
    std::vector<Latent> g2(m, lts[0]);
    std::vector<double> lml;
    double resid = 0.0;
    HIPCHK(hipMemcpyAsync(&resid, resid_dev.p, sizeof(double), hipMemcpyDeviceToHost, st0));
    if (int rc = latent_lmls(xd.p, d, n, g2.data(), lam.data(), 0, m, delta.p, lml)) return rc;   // synchronises st0
    double total = 0.0;
    for (int l = 0; l < m; ++l) total += lml[l];
    *out = total + ilmm_regulariser(n, p, m, sigma2, F.logdetST, resid);
    return LMM_OK;
  }
  F.delta(yd.p, n, delta.p);
  // one dense (mn) x (mn) factorisation: reference src/ilmm.jl:160-162 (fp32 compute mode: a Float32 matrix, as the per-latent paths)
  DenseFactor C(m * n, 1, st0);
  dense_assemble(C.A, C.D, xd.p, d, n, m, F.latd.p, ls->any_sum(), F.STd.buf.p, nullptr, delta.p, 1, st0);
  C.factor(true, st0);
  double lml = 0.0, resid = 0.0;
  HIPCHK(hipMemcpyAsync(&resid, resid_dev.p, sizeof(double), hipMemcpyDeviceToHost, st0));
  if (int rc = C.finish(&lml, st0)) return rc;
  *out = lml + ilmm_regulariser(n, p, m, sigma2, F.logdetST, resid);
  return LMM_OK;
  LMM_CATCH
}

int lmm_ilmm_logpdf(const double* x, int d, int n, const double* y, int p, const double* H, int m, double sigma2,
                    const lmm_gp_t* gps, const lmm_jitters_t* jit, double* out) {
  return lmm_ilmm_logpdf_ex(x, d, n, y, p, H, m, sigma2, gps, jit, 1, nullptr, out);
}

// logpdf(fx::FiniteGP{<:ILMM}, Y::AbstractMatrix), dense H: one value per column of Y ((n p) x ncol) from ONE (mn) x (mn)
// factorisation -- the columns ride it as rider rows (AbstractGPs.TestUtils calls logpdf(fx, Y) on ilmmx, reference
// test/ilmm.jl:34-37; the reference answers through the generic dense fallback, one factorisation per call all the same).
int lmm_ilmm_logpdf_multi(const double* x, int d, int n, const double* Y, int p, int ncol, const double* H, int m, double sigma2,
                          const lmm_gp_t* gps, const lmm_jitters_t* jit, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!x || !Y || !H || !out || d <= 0 || n <= 0 || p <= 0 || m <= 0 || ncol <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  RESOLVE(gps, m, d);
  if (!(sigma2 > 0.0)) return fail(LMM_ERR_ARG, "sigma2 must be > 0");
  if (!jit) jit = &kDefaultJit;
  if ((long long)m * n > 2000000000LL / 64) return fail(LMM_ERR_UNSUPPORTED, "m*n too large for the dense path");
  hipStream_t st0 = g.streams[0];
  DenseFront F(H, p, m);
  if (int rc = F.project(sigma2, jit->project_jitter, true)) return rc;
  DevIn xd(x, (size_t)d * n, st0), yd(Y, (size_t)n * p * ncol, st0);
  F.upload(lts, n);
  const int N = m * n;
  Buf<double> delta((size_t)N * ncol), resid_dev(ncol);
  for (int c = 0; c < ncol; ++c) {
    const double* yc = yd.p + (size_t)c * n * p;
    F.residual(yc, n, resid_dev.p + c);
    F.delta(yc, n, delta.p + (size_t)c * N);      // rider c: [latent][point]
  }
  DenseFactor C(N, ncol, st0);
  dense_assemble(C.A, C.D, xd.p, d, n, m, F.latd.p, ls->any_sum(), F.STd.buf.p, nullptr, delta.p, ncol, st0);
  C.factor(true, st0);
  std::vector<double> lml(ncol), resid(ncol);
  HIPCHK(hipMemcpyAsync(resid.data(), resid_dev.p, ncol * sizeof(double), hipMemcpyDeviceToHost, st0));
  if (int rc = C.finish(lml.data(), st0)) return rc;
  for (int c = 0; c < ncol; ++c) out[c] = lml[c] + ilmm_regulariser(n, p, m, sigma2, F.logdetST, resid[c]);
  return LMM_OK;
  LMM_CATCH
}

} // extern "C"

namespace {

struct IlmmGrad {            // host results of ilmm_grad_core
  double value = 0.0, gs2[LMM_MAX_NOISE_BLOCKS] = {};
  std::vector<double> gH;    // p x m
  std::vector<lmm_gp_grad_t> ggps;
  std::vector<double> trec;  // m x LMM_SUM_MAX_TERMS records per latent and term (grad_finish), zeros elsewhere
};

// Value and gradient of the dense-H ILMM prior logpdf over n points in NB.nblk consecutive blocks, block b carrying observation
// noise NB.s2[b].  x (d x n), y (n x p by outputs) are DEVICE pointers; gy_dev (n x p, device) may be null.  The multi-block form
// exists for the posterior's predictive density: log p(y* | y) = log p(y, y*) - log p(y)   (T y is sufficient for the latents,
// so the reference's projected posterior, src/ilmm.jl:184-198, is the exact conditional), one block per conditioning batch.
// Hblk (optional): block b is observed through the mixing matrix Hblk[b] (p x m, host) instead of H -- the latent view of a posterior
// (lmm_ilmm_post_latent_logpdf_grad_seq) observes its test block through [I_m; 0]; G.gH collects the blocks observed through H itself.
// gx_dev (optional, d x n device): d logpdf / d x from the diagonal blocks of the inverse (the latent prior is block-diagonal).
int ilmm_grad_core(const double* xd, int d, int n, const NoiseBlocks& NB, const double* yd, int p, const double* H, int m,
                   const LatentSet* ls, const lmm_jitters_t* jit, IlmmGrad& G, double* gy_dev, const double* const* Hblk = nullptr,
                   double* gx_dev = nullptr) {
  const Latent* lts = ls->lat.data();
  const int ard_d = ls->ard_grad_d();
  if ((long long)m * n > 46000) return fail(LMM_ERR_UNSUPPORTED, "m*n too large for the dense gradient (explicit (mn)^2 inverse)");
  hipStream_t st0 = g.streams[0];
  constexpr int KB = LMM_MAX_NOISE_BLOCKS;
  const int nblk = NB.nblk;
  int bi0[KB] = {}, bn[KB] = {};
  double s2[KB] = {};
  for (int b = 0; b < nblk; ++b) { bi0[b] = NB.off[b]; bn[b] = NB.count(b); s2[b] = NB.s2[b]; }
  const double* Hq[KB] = {};                       // the mixing matrix block b is observed through
  for (int b = 0; b < nblk; ++b) Hq[b] = (Hblk && Hblk[b]) ? Hblk[b] : H;
  std::vector<double> T[KB], ST[KB];
  double logdetST[KB] = {};
  for (int b = 0; b < nblk; ++b)
    if (int rc = project_dense(Hq[b], p, m, s2[b], jit->project_jitter, T[b], ST[b], &logdetST[b])) return rc;
  // host copies in the layouts the kernels read: Tt = T' (p x m), Ht = H' (m x p); the blocks' T, T', H and H' back to back
  std::vector<double> Hv, Ht, STall, Tall, Ttall;
  const std::vector<double> means = latent_means(lts, m);
  for (int b = 0; b < nblk; ++b) {
    std::vector<double> Ttb((size_t)p * m), Htb((size_t)m * p);
    for (int l = 0; l < m; ++l) for (int o = 0; o < p; ++o) { Ttb[o + (size_t)l * p] = T[b][l + (size_t)o * m]; Htb[l + (size_t)o * m] = Hq[b][o + (size_t)l * p]; }
    STall.insert(STall.end(), ST[b].begin(), ST[b].end());
    Tall.insert(Tall.end(), T[b].begin(), T[b].end());
    Ttall.insert(Ttall.end(), Ttb.begin(), Ttb.end());
    Hv.insert(Hv.end(), Hq[b], Hq[b] + (size_t)p * m);
    Ht.insert(Ht.end(), Htb.begin(), Htb.end());
  }
  std::vector<LatentDev> lat(m);
  for (int l = 0; l < m; ++l) lat[l] = lts[l].dense_dev();
  std::vector<int> sidx(n);
  for (int b = 0; b < nblk; ++b)
    for (int i = bi0[b]; i < bi0[b] + bn[b]; ++i) sidx[i] = b;
  Uploaded Tdall(Tall, st0), STd(STall, st0), Hd(Hv, st0), Ttdall(Ttall, st0), Htd(Ht, st0), meansd(means, st0);
  const double* Tdv[KB] = {};
  const double* Ttdv[KB] = {};
  const double* Hdv[KB] = {};
  const double* Htdv[KB] = {};
  for (int b = 0; b < nblk; ++b) {
    Tdv[b] = Tdall.buf.p + (size_t)b * m * p; Ttdv[b] = Ttdall.buf.p + (size_t)b * m * p;
    Hdv[b] = Hd.buf.p + (size_t)b * m * p; Htdv[b] = Htd.buf.p + (size_t)b * m * p;
  }
  Buf<LatentDev> latd(m);
  Buf<int> sidxd(n);
  HIPCHK(hipMemcpyAsync(latd.p, lat.data(), m * sizeof(LatentDev), hipMemcpyHostToDevice, st0));
  HIPCHK(hipMemcpyAsync(sidxd.p, sidx.data(), n * sizeof(int), hipMemcpyHostToDevice, st0));
  const int N = m * n;
  Buf<double> Ty((size_t)N), delta((size_t)N), partial(tall_skinny_partials(n, p)), resid_dev(KB);
  for (int b = 0; b < nblk; ++b) {
    const int i0 = bi0[b], nb_ = bn[b];
    launch_tall_skinny(yd + i0, n, nb_, p, Tdv[b], m, m, Ty.p + i0, n, nullptr, nullptr, 0, nullptr, 0, st0);
    launch_tall_skinny(yd + i0, n, nb_, p, Tdv[b], m, m, delta.p + i0, n, meansd.buf.p, nullptr, 0, nullptr, 0, st0);
    // reference src/ilmm.jl:171-181: |Y - H T Y|_F^2 of the block
    launch_tall_skinny(Ty.p + i0, n, nb_, m, Hdv[b], p, p, nullptr, 0, nullptr, yd + i0, n, partial.p, 1, st0);
    launch_sum_partials(partial.p, tall_skinny_partials(nb_, p), resid_dev.p + b, st0);
  }
  DenseFactor C(N, 1, st0);
  const Dims& D = C.D;
  Buf<double> R(mat_count((size_t)D.ld * D.NC)), alpha((size_t)D.NC);
  HIPCHK(hipMemsetAsync(alpha.p, 0, (size_t)D.NC * sizeof(double), st0));
  dense_assemble(C.A, D, xd, d, n, m, latd.p, ls->any_sum(), STd.buf.p, nblk > 1 ? sidxd.p : nullptr, delta.p, 1, st0);
  C.factor(true, st0);
  launch_extract_row(C.A, D.ld, D.NC, N, alpha.p, st0);
  backsolve1(C.A, D.ld, C.W, D.NC / 64, alpha.p, st0);
  launch_set_identity(R.p, D.ld, D.NC, st0);
  trsm_rec(R.p, D.ld, D.NC, C.A, D.ld, C.W, 0, D.NC, st0, true);                   // R = L^-T
  launch_syrk_upper_set(C.A, D.ld, R.p, D.ld, D.NC, st0);                           // lower(A) = Sigma^-1
  const int NGR = LMM_NGRAD;
  const size_t mm = (size_t)m * m, mp = (size_t)m * p;
  const std::vector<int> toff = ls->term_offsets(0, m);       // one reduction per term of every latent
  const int nterm = toff[m];
  Buf<double> red((size_t)NGR * nterm), gpart((size_t)grad_partials(n, ard_d)), Btr(KB * mm), AAt(KB * mm), AY(KB * mp);
  Buf<double> ardred((size_t)d * nterm), gxpart;
  if (gx_dev) gxpart = Buf<double>(grad_x_partial_elems(n, d));
  for (int l = 0; l < m; ++l) {
    const double* Kl = mat_at(C.A, (size_t)l * n * D.ld + (size_t)l * n);
    for (int c = 0; c < lts[l].nt(); ++c) {
      const LatentDev& gd = lts[l].terms[c].gd;
      const size_t t = (size_t)toff[l] + c;
      launch_grad_reduce(Kl, D.ld, n, n, alpha.p + (size_t)l * n, delta.p + (size_t)l * n, xd, d, gd, gpart.p, red.p + NGR * t, st0,
                         ardred.p + d * t);
      if (gx_dev) launch_grad_x(Kl, D.ld, n, alpha.p + (size_t)l * n, xd, d, gd, gxpart.p, gx_dev, l > 0 || c > 0, st0);
    }
  }
  // regulariser pieces: Rm = Y - (T Y)' H' (n x p), RH = Rm H (n x m), per block Rm' Ty (p x m), RH' Y (m x p)
  Buf<double> HTY((size_t)n * p), Rm((size_t)n * p), RH((size_t)N), RtTy(KB * mp), RHtY(KB * mp);
  for (int b = 0; b < nblk; ++b)
    launch_tall_skinny(Ty.p + bi0[b], n, bn[b], m, Hdv[b], p, p, HTY.p + bi0[b], n, nullptr, nullptr, 0, nullptr, 0, st0);
  launch_vec_lin(yd, HTY.p, -1.0, n * p, Rm.p, st0);
  for (int b = 0; b < nblk; ++b)
    launch_tall_skinny(Rm.p + bi0[b], n, bn[b], p, Htdv[b], m, m, RH.p + bi0[b], n, nullptr, nullptr, 0, nullptr, 0, st0);
  for (int b = 0; b < nblk; ++b) {
    const int i0 = bi0[b], nb_ = bn[b];
    launch_block_trace(C.A, D.ld, n, m, i0, i0 + nb_, Btr.p + b * mm, st0);
    launch_atb(alpha.p + i0, n, alpha.p + i0, n, nb_, m, m, AAt.p + b * mm, st0);      // (alpha_l . alpha_l') over the block
    launch_atb(alpha.p + i0, n, yd + i0, n, nb_, m, p, AY.p + b * mp, st0);            // sum_i alpha_l[i] Y[i, o]   (m x p)
    launch_atb(Rm.p + i0, n, Ty.p + i0, n, nb_, p, m, RtTy.p + b * mp, st0);
    launch_atb(RH.p + i0, n, yd + i0, n, nb_, m, p, RHtY.p + b * mp, st0);
  }
  std::vector<double> hred((size_t)NGR * nterm), hB(KB * mm), hAAt(KB * mm), hAY(KB * mp), hRtTy(KB * mp), hRHtY(KB * mp);
  double lml = 0.0, resid[KB] = {};
  HIPCHK(hipMemcpyAsync(resid, resid_dev.p, nblk * sizeof(double), hipMemcpyDeviceToHost, st0));
  HIPCHK(hipMemcpyAsync(hred.data(), red.p, hred.size() * sizeof(double), hipMemcpyDeviceToHost, st0));
  std::vector<double> hard(ard_d ? (size_t)d * nterm : 0, 0.0);
  if (!hard.empty()) HIPCHK(hipMemcpyAsync(hard.data(), ardred.p, hard.size() * sizeof(double), hipMemcpyDeviceToHost, st0));
  HIPCHK(hipMemcpyAsync(hB.data(), Btr.p, nblk * mm * sizeof(double), hipMemcpyDeviceToHost, st0));
  HIPCHK(hipMemcpyAsync(hAAt.data(), AAt.p, nblk * mm * sizeof(double), hipMemcpyDeviceToHost, st0));
  HIPCHK(hipMemcpyAsync(hAY.data(), AY.p, nblk * mp * sizeof(double), hipMemcpyDeviceToHost, st0));
  HIPCHK(hipMemcpyAsync(hRtTy.data(), RtTy.p, nblk * mp * sizeof(double), hipMemcpyDeviceToHost, st0));
  HIPCHK(hipMemcpyAsync(hRHtY.data(), RHtY.p, nblk * mp * sizeof(double), hipMemcpyDeviceToHost, st0));
  if (int rc = C.finish(&lml, st0)) return rc;
  // value: reference src/ilmm.jl:150-163 + :171-181
  G.value = lml;
  for (int b = 0; b < nblk; ++b)
    G.value += ilmm_regulariser(bn[b], p, m, s2[b], logdetST[b], resid[b]);
  // ---- kernel-parameter gradients: 1/2 tr((aa' - Sigma^-1) dSigma/dtheta_l), dSigma = E_ll (x) dK_l ----
  G.ggps.assign(m, lmm_gp_grad_t{});
  G.trec.assign((size_t)m * LMM_SUM_MAX_TERMS * term_grad_stride(d), 0.0);
  for (int l = 0; l < m; ++l) {                     // the trace, a.a and sum-of-alpha partials from term 0's reduction; K_ii = kappa(0)
    const double* r = &hred[(size_t)NGR * toff[l]];
    G.ggps[l].lengthscale = grad_finish(lts[l], d, r, hard.empty() ? nullptr : &hard[(size_t)d * toff[l]], r[2], r[1],
                                        &G.trec[(size_t)l * LMM_SUM_MAX_TERMS * term_grad_stride(d)], &G.ggps[l].variance);
    G.ggps[l].mean = r[4];
  }
  // ---- per block: the cotangents of its T (m x p) and SigmaT (m x m), then backward through project(H_b, sigma2_b) ----
  G.gH.assign(mp, 0.0);
  for (int b = 0; b < nblk; ++b) {
    const double s = 1.0 / s2[b];
    const double* bAY = &hAY[b * mp]; const double* bRHtY = &hRHtY[b * mp]; const double* bRtTy = &hRtTy[b * mp];
    const double* bAAt = &hAAt[b * mm]; const double* bB = &hB[b * mm];
    std::vector<double> Tb(mp), Gs(mm), Hb(mp, 0.0);      // Hb: kept only for the blocks observed through the model's H
    for (size_t q = 0; q < mp; ++q) Tb[q] = -bAY[q] + s * bRHtY[q];            // lml + regulariser (residual)
    // SigmaT^-1 for the +n/2 logdet SigmaT term of the regulariser
    std::vector<double> STc = ST[b], STinv(mm, 0.0);
    if (!host_cholesky(STc, m)) return fail(LMM_ERR_NOT_PD, "PosDefException: SigmaT not PD");
    for (int l = 0; l < m; ++l) STinv[l + (size_t)l * m] = 1.0;
    host_chol_solve(STc, m, STinv.data(), m);
    for (size_t q = 0; q < mm; ++q) Gs[q] = 0.5 * (bAAt[q] - bB[q]) + 0.5 * (double)bn[b] * STinv[q];
    // explicit sigma2 of the regulariser and explicit H of the residual
    double s2g = 0.0;
    s2g += -0.5 * ((double)bn[b] * (double)p / s2[b] - resid[b] / (s2[b] * s2[b]));
    for (size_t q = 0; q < mp; ++q) Hb[q] += s * bRtTy[q];
    if (int rc = project_dense_backward(Hq[b], p, m, s2[b], jit->project_jitter, T[b], Tb, Gs, Hb, s2g)) return rc;
    G.gs2[b] = s2g;
    if (!(Hblk && Hblk[b])) for (size_t q = 0; q < mp; ++q) G.gH[q] += Hb[q];
  }
  if (gy_dev) {
    // dL/dY (n x p) = -((alpha - RH / sigma2_i) T_i) - Rm / sigma2_i     (alpha as the n x m matrix [point][latent])
    Buf<double> Z((size_t)N), ZT((size_t)n * p);
    launch_vec_lin_blocks(alpha.p, RH.p, NB, -1.0, n, (size_t)N, Z.p, st0);
    for (int b = 0; b < nblk; ++b)
      launch_tall_skinny(Z.p + bi0[b], n, bn[b], m, Ttdv[b], p, p, ZT.p + bi0[b], n, nullptr, nullptr, 0, nullptr, 0, st0);
    launch_vec_lin_blocks(ZT.p, Rm.p, NB, 1.0, n, (size_t)n * p, ZT.p, st0);
    launch_vec_axpby(ZT.p, -1.0, ZT.p, 0.0, (size_t)n * p, gy_dev, st0);
    HIPCHK(hipStreamSynchronize(st0));
  }
  return LMM_OK;
}

}  // namespace

extern "C" {

// Value and gradient of logpdf(fx::FiniteGP{<:ILMM}, y) with a dense H (reference src/ilmm.jl:150-181 differentiated; the
// reference's tests take Zygote.gradient(logpdf, ilmmx, y), test/ilmm.jl:31) w.r.t. y, sigma2, H (p x m) and every latent's
// (variance, lengthscale, mean).  The reference's own operation: ONE (mn) x (mn) factorisation of blockdiag(K_l) + SigmaT (x) I;
// here additionally its explicit inverse (triangular solve of identity riders + upper-triangular SYRK on the MFMA kernels),
// per-latent contractions on the diagonal blocks of the inverse, and the chain rule through project(H, sigma2)
// (src/ilmm.jl:61-68) and the regulariser (src/ilmm.jl:171-181) as small host algebra.  Does not shard.
int lmm_ilmm_logpdf_grad_x(const double* x, int d, int n, const double* y, int p, const double* H, int m, double sigma2,
                           const lmm_gp_t* gps, const lmm_jitters_t* jit, double* out_logpdf, double* grad_y, double* grad_sigma2,
                           double* grad_H, lmm_gp_grad_t* grad_gps, double* grad_x) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!x || !y || !H || !out_logpdf || d <= 0 || n <= 0 || p <= 0 || m <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  RESOLVE(gps, m, d);
  if (!(sigma2 > 0.0)) return fail(LMM_ERR_ARG, "sigma2 must be > 0");
  if (!jit) jit = &kDefaultJit;
  hipStream_t st0 = g.streams[0];
  DevIn xd(x, (size_t)d * n, st0), yd(y, (size_t)n * p, st0);
  DevOut gy(grad_y, (size_t)n * p), gx(grad_x, (size_t)d * n);
  if (int rc = ls->ard_grad_check()) return rc;
  if (int rc = input_grad_check(d, grad_x != nullptr)) return rc;
  if (grad_x) { if (int rc = refuse_sho(*ls, "gradients with respect to the inputs are")) return rc; }
  IlmmGrad G;
  if (int rc = ilmm_grad_core(xd.p, d, n, one_noise_block(n, sigma2), yd.p, p, H, m, ls.get(), jit, G, gy.p, nullptr, gx.p)) return rc;
  publish_grads(*ls, grad_gps ? &G.trec : nullptr, 0, m);
  *out_logpdf = G.value;
  if (grad_sigma2) *grad_sigma2 = G.gs2[0];
  if (grad_H) std::copy(G.gH.begin(), G.gH.end(), grad_H);
  if (grad_gps) for (int l = 0; l < m; ++l) grad_gps[l] = G.ggps[l];
  if (grad_y) gy.finish(st0);
  if (grad_x) gx.finish(st0);
  if (grad_y || grad_x) HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

int lmm_ilmm_logpdf_grad(const double* x, int d, int n, const double* y, int p, const double* H, int m, double sigma2,
                         const lmm_gp_t* gps, const lmm_jitters_t* jit, double* out_logpdf, double* grad_y, double* grad_sigma2,
                         double* grad_H, lmm_gp_grad_t* grad_gps) {
  return lmm_ilmm_logpdf_grad_x(x, d, n, y, p, H, m, sigma2, gps, jit, out_logpdf, grad_y, grad_sigma2, grad_H, grad_gps, nullptr);
}

// Value and TOTAL derivatives of logpdf(posterior(f(x, sigma2), y)(xs, sigma2_s), ys) for the dense-H ILMM -- what
// Zygote.gradient(logpdf, pi, y_test) differentiates in reference test/ilmm.jl:32 -- as the joint prior density of (y, ys) under
// per-block noise minus the prior density of y.  Does not shard.  _seq: sequentially conditioned posterior (src/ilmm.jl:184-198
// applied to its own result), one noise block per conditioning batch; x, y as in lmm_oilmm_post_logpdf_grad_seq.
}  // extern "C"

namespace {
// latent_test: the test block observes the LATENT processes (ys is ns x m): get_latent_gp(posterior)(xs, sigma2_s)
int ilmm_post_logpdf_grad_impl(bool latent_test, const double* x, int d, int n, const int* batch_n, const double* batch_sigma2, int nbatch,
                               const double* y, const double* xs, int ns, const double* ys, int p, const double* H, int m,
                               double sigma2_s, const lmm_gp_t* gps, const lmm_jitters_t* jit, double* out_logpdf, double* grad_y,
                               double* grad_ys, double* grad_batch_sigma2, double* grad_sigma2_s, double* grad_H,
                               lmm_gp_grad_t* grad_gps, double* grad_x, double* grad_xs) {
  if (!x || !y || !xs || !ys || !H || !out_logpdf || d <= 0 || n <= 0 || ns <= 0 || p <= 0 || m <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  if (latent_test && m > p) return fail(LMM_ERR_DIM, "out dim of x != out dim of f.");
  RESOLVE(gps, m, d);
  if (int rc = check_batches(batch_n, batch_sigma2, nbatch, n)) return rc;
  if (!(sigma2_s > 0.0)) return fail(LMM_ERR_ARG, "sigma2 must be > 0");
  if (!jit) jit = &kDefaultJit;
  hipStream_t st0 = g.streams[0];
  DevIn xd(x, (size_t)d * n, st0), yd(y, (size_t)n * p, st0);
  // The latent view observes its test points through H* = [I_m; 0] (p x m): z embedded in the first m of p output columns.  project(H*,
  // s) gives T = [I 0], SigmaT = s I (src/ilmm.jl:61-68) -- the latent FiniteGP's own noise -- and a residual of 0; what the p - m
  // padded columns add to the regulariser, -ns (p - m) log(2 pi s) / 2, is taken out again below.
  std::vector<double> Hlat;
  const double* Hblk[LMM_MAX_NOISE_BLOCKS] = {};
  if (latent_test) {
    Hlat.assign((size_t)p * m, 0.0);
    for (int l = 0; l < m; ++l) Hlat[l + (size_t)l * p] = 1.0;
    Hblk[nbatch] = Hlat.data();
  }
  IlmmGrad GJ, GM;
  auto core = [&](bool joint, const double* xq, int nq, const NoiseBlocks& NB, const double* yq, IlmmGrad& G, double* gy, double* gx) {
    return ilmm_grad_core(xq, d, nq, NB, yq, p, H, m, ls.get(), jit, G, gy, joint && latent_test ? Hblk : nullptr, gx);
  };
  if (int rc = predictive_grad(*ls, 0, m, xd.p, yd.p, d, n, batch_n, batch_sigma2, nbatch, xs, ns, ys, p, latent_test ? m : p, sigma2_s, core,
                               GJ, GM, grad_y, grad_ys, grad_batch_sigma2, grad_gps, grad_x, grad_xs)) return rc;
  const double pad = latent_test ? 0.5 * (double)ns * (double)(p - m) : 0.0;
  *out_logpdf = GJ.value - GM.value + pad * (kLog2Pi + std::log(sigma2_s));
  if (grad_sigma2_s) *grad_sigma2_s = GJ.gs2[nbatch] + pad / sigma2_s;
  if (grad_H) for (size_t q = 0; q < (size_t)p * m; ++q) grad_H[q] = GJ.gH[q] - GM.gH[q];
  return LMM_OK;
}
}  // namespace

extern "C" {

int lmm_ilmm_post_logpdf_grad_seq_x(const double* x, int d, int n, const int* batch_n, const double* batch_sigma2, int nbatch,
                                    const double* y, const double* xs, int ns, const double* ys, int p, const double* H, int m,
                                    double sigma2_s, const lmm_gp_t* gps, const lmm_jitters_t* jit, double* out_logpdf, double* grad_y,
                                    double* grad_ys, double* grad_batch_sigma2, double* grad_sigma2_s, double* grad_H,
                                    lmm_gp_grad_t* grad_gps, double* grad_x, double* grad_xs) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  return ilmm_post_logpdf_grad_impl(false, x, d, n, batch_n, batch_sigma2, nbatch, y, xs, ns, ys, p, H, m, sigma2_s, gps, jit, out_logpdf,
                                    grad_y, grad_ys, grad_batch_sigma2, grad_sigma2_s, grad_H, grad_gps, grad_x, grad_xs);
  LMM_CATCH
}

int lmm_ilmm_post_logpdf_grad_seq(const double* x, int d, int n, const int* batch_n, const double* batch_sigma2, int nbatch,
                                  const double* y, const double* xs, int ns, const double* ys, int p, const double* H, int m,
                                  double sigma2_s, const lmm_gp_t* gps, const lmm_jitters_t* jit, double* out_logpdf, double* grad_y,
                                  double* grad_ys, double* grad_batch_sigma2, double* grad_sigma2_s, double* grad_H,
                                  lmm_gp_grad_t* grad_gps) {
  return lmm_ilmm_post_logpdf_grad_seq_x(x, d, n, batch_n, batch_sigma2, nbatch, y, xs, ns, ys, p, H, m, sigma2_s, gps, jit, out_logpdf,
                                         grad_y, grad_ys, grad_batch_sigma2, grad_sigma2_s, grad_H, grad_gps, nullptr, nullptr);
}

// The same for the LATENT view of the posterior: logpdf(get_latent_gp(posterior(...))(xs, sigma2_s), zs) with zs (ns x m, by outputs over
// the m latents) -- reference src/ilmm.jl:39 on the posterior ILMM of :196-197, whose latent GP is the coupled PosteriorGP of the
// IndependentMOGP; Zygote differentiates its logpdf like any other.  grad_ys: ns x m.  grad_H: through the conditioning batches only.
int lmm_ilmm_post_latent_logpdf_grad_seq_x(const double* x, int d, int n, const int* batch_n, const double* batch_sigma2, int nbatch,
                                           const double* y, const double* xs, int ns, const double* zs, int p, const double* H, int m,
                                           double sigma2_s, const lmm_gp_t* gps, const lmm_jitters_t* jit, double* out_logpdf,
                                           double* grad_y, double* grad_zs, double* grad_batch_sigma2, double* grad_sigma2_s,
                                           double* grad_H, lmm_gp_grad_t* grad_gps, double* grad_x, double* grad_xs) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  return ilmm_post_logpdf_grad_impl(true, x, d, n, batch_n, batch_sigma2, nbatch, y, xs, ns, zs, p, H, m, sigma2_s, gps, jit, out_logpdf,
                                    grad_y, grad_zs, grad_batch_sigma2, grad_sigma2_s, grad_H, grad_gps, grad_x, grad_xs);
  LMM_CATCH
}

int lmm_ilmm_post_latent_logpdf_grad_seq(const double* x, int d, int n, const int* batch_n, const double* batch_sigma2, int nbatch,
                                         const double* y, const double* xs, int ns, const double* zs, int p, const double* H, int m,
                                         double sigma2_s, const lmm_gp_t* gps, const lmm_jitters_t* jit, double* out_logpdf, double* grad_y,
                                         double* grad_zs, double* grad_batch_sigma2, double* grad_sigma2_s, double* grad_H,
                                         lmm_gp_grad_t* grad_gps) {
  return lmm_ilmm_post_latent_logpdf_grad_seq_x(x, d, n, batch_n, batch_sigma2, nbatch, y, xs, ns, zs, p, H, m, sigma2_s, gps, jit,
                                                out_logpdf, grad_y, grad_zs, grad_batch_sigma2, grad_sigma2_s, grad_H, grad_gps, nullptr,
                                                nullptr);
}

// One conditioning batch: posterior(f(x, sigma2), y).
int lmm_ilmm_post_logpdf_grad(const double* x, int d, int n, const double* y, const double* xs, int ns, const double* ys, int p,
                              const double* H, int m, double sigma2, double sigma2_s, const lmm_gp_t* gps, const lmm_jitters_t* jit,
                              double* out_logpdf, double* grad_y, double* grad_ys, double* grad_sigma2, double* grad_sigma2_s,
                              double* grad_H, lmm_gp_grad_t* grad_gps) {
  return lmm_ilmm_post_logpdf_grad_seq(x, d, n, &n, &sigma2, 1, y, xs, ns, ys, p, H, m, sigma2_s, gps, jit, out_logpdf, grad_y, grad_ys,
                                       grad_sigma2, grad_sigma2_s, grad_H, grad_gps);
}

// ------------------------------------------------------------------------------------------------
// posterior
// ------------------------------------------------------------------------------------------------
// noise: per-latent scalar (host, indexed by latent) used when noisevec == NULL; noisevec: device [k][n] per-point noise.
static int posterior_create_common(const double* xd, int d, int n, std::shared_ptr<LatentSet> ls, const double* noise,
                                   int l0, int l1, const double* delta, lmm_post_t** out, const double* noisevec = nullptr) {
  const int m = (int)ls->lat.size();
  const Latent* lts = ls->lat.data();
  const int ms = l1 - l0, mk = std::max(ms, 1);
  lmm_post* P = new lmm_post();
  try {
    Dims D(n, 1);
    P->kind = 0; P->f32 = g_f32; P->n = n; P->d = d; P->l0 = l0; P->l1 = l1; P->m = m;
    P->NC = D.NC; P->NR = D.NR; P->ld = D.ld;
    P->ls = std::move(ls);
    P->x = Buf<double>((size_t)d * n);
    HIPCHK(hipMemcpyAsync(P->x.p, xd, (size_t)d * n * sizeof(double), hipMemcpyDeviceToDevice, g.streams[0]));
    FanOut F(ms, mat_bytes((double)D.elems()));
    int* info = F.alloc_info();
    for (int k = 0; k < ms; ++k) {
      P->L.emplace_back(mat_count((size_t)D.elems()));
      P->W.emplace_back(mat_count((size_t)(D.NC / 64) * 4096));
      P->alpha.emplace_back((size_t)D.NC);
      P->z.emplace_back((size_t)D.NC);
    }
    P->delta_all = Buf<double>((size_t)n * mk);
    if (ms > 0) HIPCHK(hipMemcpyAsync(P->delta_all.p, delta, (size_t)n * ms * sizeof(double), hipMemcpyDeviceToDevice, g.streams[0]));
    if (noisevec) {
      P->noise_all = Buf<double>((size_t)n * mk);
      if (ms > 0) HIPCHK(hipMemcpyAsync(P->noise_all.p, noisevec, (size_t)n * ms * sizeof(double), hipMemcpyDeviceToDevice, g.streams[0]));
    } else {
      P->noise_scalar.assign(noise + l0, noise + l1);
    }
    F.run([&](const FanBatch& b) {
      hipStream_t st = b.st;
      const int nb = b.nb;
      Batch B;
      GramArgs ga[LMM_MAX_BATCH];
      for (int j = 0; j < nb; ++j) {
        const int k = b.k0 + j;
        ga[j] = train_gram_args(lts[l0 + k], P->x.p, d, n, D, P->L[k].p, noisevec ? 0.0 : noise[l0 + k],
                                noisevec ? P->noise_all.p + (size_t)k * n : nullptr, delta + (size_t)k * n, 1);
        B.add(P->L[k].p, P->W[k].p, info + k);
      }
      {
        const double gb = train_gram_bytes(n);
        ProfScope ps(LMM_PROF_GRAM, nb * gb, st, 0, 0, 0, nb * gb, nb);
        gram_batch_g(ga, nb, st);
      }
      potrf_batch(B, D.ld, D.NR, D.NC, n, st, D.NC + 1);        // one rider row (delta); rows NC + 1 .. NR - 1 are zero padding
      // alpha = L^-T (L^-1 delta): the rider row is z = L^-1 delta (kept as P->z, zero-padded to NC)
      BatchPtr ab{}, zb{};
      for (int j = 0; j < nb; ++j) { ab.p[j] = P->alpha[b.k0 + j].p; zb.p[j] = P->z[b.k0 + j].p; }
      launch_extract_rows(B.A, nb, D.ld, D.NC, n, D.NC, ab, zb, st);
      launch_backsolve(B.A, D.ld, B.W, D.NC / 64, ab, nb, st);
    });
    if (int rc = F.check(l0)) { delete P; return rc; }
  } catch (int code) { drain_after_error(); delete P; return code; }
  *out = P;
  return LMM_OK;
}

int lmm_oilmm_posterior_create(const double* x, int d, int n, const double* y, int p, const double* U, const double* S,
                               int m, double sigma2, const lmm_gp_t* gps, int latent_begin, int latent_end,
                               lmm_post_t** out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  Train R;
  if (int rc = train(!x || !y || !U || !S || !out || d <= 0 || n <= 0 || p <= 0 || m <= 0, x, d, n, y, (size_t)n * p, p, S, m, sigma2, gps, latent_begin,
                     latent_end, 0, R)) return rc;
  OilmmFront F(U, S, p, m, sigma2);
  F.upload(R.means);
  Buf<double> delta = F.delta(R.yd.p, n, R.l0, R.ms);
  return posterior_create_common(R.xd.p, d, n, R.ls, F.ST.data(), latent_begin, latent_end, delta.p, out);
  LMM_CATCH
}

// posterior(po(x2, sigma2), y2) -- conditioning a posterior OILMM / IndependentMOGP on further observations (exercised by
// AbstractGPs.TestUtils on `po` in reference test/oilmm.jl:34-37; AbstractGPs updates the Cholesky factor).  Latent by
// latent the result is the posterior of the PRIOR given both data sets, each with its own projected noise, so the new state is
// built from the concatenated inputs, the kept residuals and per-point noise.  U, S: the mixing matrix (U = I, S = 1 for a
// bare IndependentMOGP, with p == m).
int lmm_post_condition(const lmm_post_t* post, const double* U, const double* S, int p, int m, double sigma2,
                       const double* x2, int d, int n2, const double* y2, lmm_post_t** out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (int rc = post_dtype_check(post)) return rc;
  if (!post || !U || !S || !x2 || !y2 || !out || d <= 0 || n2 <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  const lmm_post* P = post;
  Shard Q;
  if (int rc = post_shard(P, "sequential conditioning of the dense-H posterior is not built", nullptr, m, d, 0, 0, Q)) return rc;
  if (m > p) return fail(LMM_ERR_DIM, "out dim of x != out dim of f.");
  hipStream_t st0 = g.streams[0];
  const int l0 = Q.l0, l1 = Q.l1, ms = Q.ms, n1 = P->n, n = n1 + n2;
  OilmmFront F(U, S, p, m, sigma2);
  const std::vector<double>& ST = F.ST;
  DevIn x2d(x2, (size_t)d * n2, st0), y2d(y2, (size_t)n2 * p, st0);
  const std::vector<double> means = latent_means(Q.lts, m);
  F.upload(means);
  Buf<double> xall((size_t)d * n), delta((size_t)n * Q.mk), nv((size_t)n * Q.mk);
  HIPCHK(hipMemcpyAsync(xall.p, P->x.p, (size_t)d * n1 * sizeof(double), hipMemcpyDeviceToDevice, st0));
  HIPCHK(hipMemcpyAsync(xall.p + (size_t)d * n1, x2d.p, (size_t)d * n2 * sizeof(double), hipMemcpyDeviceToDevice, st0));
  Buf<double> d2buf = F.delta(y2d.p, n2, l0, ms);
  for (int k = 0; k < ms; ++k) {
    HIPCHK(hipMemcpyAsync(delta.p + (size_t)k * n, P->delta_all.p + (size_t)k * n1, (size_t)n1 * sizeof(double), hipMemcpyDeviceToDevice, st0));
    HIPCHK(hipMemcpyAsync(delta.p + (size_t)k * n + n1, d2buf.p + (size_t)k * n2, (size_t)n2 * sizeof(double), hipMemcpyDeviceToDevice, st0));
    if (P->noise_all.p != nullptr)
      HIPCHK(hipMemcpyAsync(nv.p + (size_t)k * n, P->noise_all.p + (size_t)k * n1, (size_t)n1 * sizeof(double), hipMemcpyDeviceToDevice, st0));
    else launch_fill(nv.p + (size_t)k * n, n1, P->noise_scalar[k], st0);
    launch_fill(nv.p + (size_t)k * n + n1, n2, ST[l0 + k], st0);
  }
  return posterior_create_common(xall.p, d, n, P->ls, ST.data(), l0, l1, delta.p, out, nv.p);
  LMM_CATCH
}

// ------------------------------------------------------------------------------------------------
// missing observations (NaN in y): the diagonal approximation of the OILMM paper (Bruinsma et al. 2020) for missing data, which
// the reference's notebook names as not yet supported ("Heterotopic and missing data ... are not supported yet").  DESIGN.md 4.15.
// Per point t with observed outputs O_t: H_t = H[O_t, :], G_t = H_t' H_t, z_t = G_t^-1 H_t' y_t[O_t]; latent l sees z_t[l] with noise
// sigma2 (G_t^-1)_ll; the regulariser gains -1/2 [(p_t - m) log(2 pi sigma2) + log det G_t + |y_t[O_t] - H_t z_t|^2 / sigma2].
// ------------------------------------------------------------------------------------------------
// Groups the points' masks (nw words each) into patterns numbered by first appearance.  A point with fewer than m observed outputs
// is refused (LMM_ERR_UNSUPPORTED, the 0-based point index in the error detail's `info`).
static int missing_group(const unsigned long long* masks, int n, int m, int nw, std::vector<int>& pat_of,
                         std::vector<unsigned long long>& pmask, std::vector<int>& first_point, long long* n_observed) {
  std::unordered_map<std::string, int> seen;
  pat_of.resize(n); pmask.clear(); first_point.clear();
  long long tot = 0;
  for (int t = 0; t < n; ++t) {
    const unsigned long long* mk = masks + (size_t)t * nw;
    int pt = 0;
    for (int w = 0; w < nw; ++w) pt += __builtin_popcountll(mk[w]);
    if (pt < m) {
      g.err_latent = -1; g.err_info = t;
      if (pt == 0) return fail(LMM_ERR_UNSUPPORTED, "missing data: point %d has no observed output (drop it before the call)", t);
      return fail(LMM_ERR_UNSUPPORTED, "missing data: point %d observes %d outputs, fewer than the m = %d latent processes", t, pt, m);
    }
    tot += pt;
    const auto ins = seen.emplace(std::string(reinterpret_cast<const char*>(mk), (size_t)nw * sizeof(unsigned long long)), (int)first_point.size());
    if (ins.second) { pmask.insert(pmask.end(), mk, mk + nw); first_point.push_back(t); }
    pat_of[t] = ins.first->second;
  }
  if (n_observed) *n_observed = tot;
  return LMM_OK;
}

int lmm_missing_patterns(const double* y_host, int n, int p, int m, int* pattern_of_point, int* npatterns, int* n_observed) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!y_host || n <= 0 || p <= 0 || m <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  const int nw = (p + 63) / 64;
  std::vector<unsigned long long> masks((size_t)n * nw, 0ull);
  for (int o = 0; o < p; ++o)
    for (int t = 0; t < n; ++t) {
      const double v = y_host[t + (size_t)o * n];
      if (v == v) masks[(size_t)t * nw + (o >> 6)] |= 1ull << (o & 63);
    }
  std::vector<int> pat_of, first_point;
  std::vector<unsigned long long> pmask;
  long long tot = 0;
  if (int rc = missing_group(masks.data(), n, m, nw, pat_of, pmask, first_point, &tot)) return rc;
  if (pattern_of_point) std::copy(pat_of.begin(), pat_of.end(), pattern_of_point);
  if (npatterns) *npatterns = (int)first_point.size();
  if (n_observed) *n_observed = (int)std::min<long long>(tot, 2147483647LL);
  return LMM_OK;
}

// Device state of the front end for one call: the patterns, their projections and the per-latent pseudo-observations of the shard.
struct MissingFront {
  int npat = 0;
  Buf<int> pat_of;
  Buf<unsigned long long> pmask;
  Buf<double> Hd, Tpat, dinv, z, nv, resid;      // z, nv: [latent of the shard][n] (z - mean, sigma2 (G_t^-1)_ll); resid: n x p or empty
  double rss = 0.0, sum_pt = 0.0, sum_logdet = 0.0;
  // sum_t r_t
  double reg(int n, int m, double s2) const {
    return -0.5 * ((sum_pt - (double)n * m) * std::log(2.0 * M_PI * s2) + sum_logdet + rss / s2);
  }
};

// yd: n x p (device; NaN = missing, never downloaded: only the n * nw mask words are).  means: m host values or nullptr.  Returns with
// streams[0] drained.  A G_t that is not positive definite: LMM_ERR_NOT_PD with the first such point in the detail's `info`.
static int missing_front(const double* yd, int n, int p, const double* U, const double* S, int m, double s2, const double* means,
                         int l0, int l1, bool want_resid, MissingFront& F) {
  if (m > LMM_MISSING_MMAX) return fail(LMM_ERR_UNSUPPORTED, "missing data is served for m <= %d latent processes (m = %d)", LMM_MISSING_MMAX, m);
  hipStream_t st0 = g.streams[0];
  const int nw = (p + 63) / 64, ms = l1 - l0;
  Buf<unsigned long long> masks((size_t)n * nw);
  Buf<int> pt(n);
  launch_missing_masks(yd, n, p, masks.p, pt.p, st0);
  std::vector<unsigned long long> hmasks((size_t)n * nw), pmask;
  HIPCHK(hipMemcpyAsync(hmasks.data(), masks.p, hmasks.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st0));
  HIPCHK(hipStreamSynchronize(st0));
  std::vector<int> pat_of, first_point;
  if (int rc = missing_group(hmasks.data(), n, m, nw, pat_of, pmask, first_point, nullptr)) return rc;
  const int npat = (int)first_point.size();
  F.npat = npat;
  F.pat_of = Buf<int>(n); F.pmask = Buf<unsigned long long>(pmask.size());
  HIPCHK(hipMemcpyAsync(F.pat_of.p, pat_of.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st0));
  HIPCHK(hipMemcpyAsync(F.pmask.p, pmask.data(), pmask.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st0));
  const std::vector<double> Hh = shard_H(U, S, p, 0, m);          // reference src/orthogonal_matrix.jl:27-30
  F.Hd = Buf<double>(Hh.size());
  HIPCHK(hipMemcpyAsync(F.Hd.p, Hh.data(), Hh.size() * sizeof(double), hipMemcpyHostToDevice, st0));
  Buf<double> meansd(m);
  if (means) HIPCHK(hipMemcpyAsync(meansd.p, means, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st0));
  F.Tpat = Buf<double>((size_t)npat * m * p); F.dinv = Buf<double>((size_t)npat * m);
  F.z = Buf<double>((size_t)n * std::max(ms, 1)); F.nv = Buf<double>((size_t)n * std::max(ms, 1));
  if (want_resid) F.resid = Buf<double>((size_t)n * p);
  Buf<double> scratch(missing_pattern_scratch_elems(m, npat)), logdet(npat), part(3 * (size_t)n), sums(3);
  Buf<int> info(npat);
  launch_missing_patterns(F.Hd.p, p, m, F.pmask.p, npat, scratch.p, F.Tpat.p, F.dinv.p, logdet.p, info.p, st0);
  launch_missing_apply(yd, n, p, m, F.pat_of.p, F.pmask.p, F.Tpat.p, F.dinv.p, logdet.p, pt.p, F.Hd.p, s2, means ? meansd.p : nullptr,
                       l0, l1, F.z.p, F.nv.p, want_resid ? F.resid.p : nullptr, part.p, sums.p, st0);
  std::vector<int> hinfo(npat);
  double hs[3] = {0.0, 0.0, 0.0};
  HIPCHK(hipMemcpyAsync(hinfo.data(), info.p, (size_t)npat * sizeof(int), hipMemcpyDeviceToHost, st0));
  HIPCHK(hipMemcpyAsync(hs, sums.p, sizeof hs, hipMemcpyDeviceToHost, st0));
  HIPCHK(hipStreamSynchronize(st0));
  for (int q = 0; q < npat; ++q)
    if (hinfo[q] != 0) {       // patterns are numbered by first appearance: this is the first point with a singular G_t
      g.err_latent = -1; g.err_info = first_point[q];
      return fail(LMM_ERR_NOT_PD, "PosDefException: H_t' H_t of point %d is not positive definite over its observed outputs (pivot %d)",
                  first_point[q], hinfo[q]);
    }
  F.rss = hs[0]; F.sum_pt = hs[1]; F.sum_logdet = hs[2];
  return LMM_OK;
}

int lmm_oilmm_project_missing(const double* y, int n, int p, const double* U, const double* S, int m, double sigma2,
                              const double* means, double* z_out, double* noise_out, double* reg_out, int* npatterns_out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (int rc = train_args(!y || !U || !S || n <= 0 || p <= 0 || m <= 0, p, m, S, sigma2, 0, m, TRAIN_SIGMA2 | TRAIN_S)) return rc;
  hipStream_t st0 = g.streams[0];
  DevIn yd(y, (size_t)n * p, st0);
  MissingFront F;
  if (int rc = missing_front(yd.p, n, p, U, S, m, sigma2, means, 0, m, false, F)) return rc;
  DevOut zo(z_out, (size_t)n * m), no(noise_out, (size_t)n * m);
  if (z_out) HIPCHK(hipMemcpyAsync(zo.p, F.z.p, (size_t)n * m * sizeof(double), hipMemcpyDeviceToDevice, st0));
  if (noise_out) HIPCHK(hipMemcpyAsync(no.p, F.nv.p, (size_t)n * m * sizeof(double), hipMemcpyDeviceToDevice, st0));
  zo.finish(st0); no.finish(st0);
  HIPCHK(hipStreamSynchronize(st0));
  if (reg_out) *reg_out = F.reg(n, m, sigma2);
  if (npatterns_out) *npatterns_out = F.npat;
  return LMM_OK;
  LMM_CATCH
}

int lmm_oilmm_logpdf_missing(const double* x, int d, int n, const double* y, int p, const double* U, const double* S, int m,
                             double sigma2, const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  Train R;
  if (int rc = train(!x || !y || !U || !S || !out || d <= 0 || n <= 0 || p <= 0 || m <= 0, x, d, n, y, (size_t)n * p, p, S, m, sigma2, gps, latent_begin,
                     latent_end, TRAIN_SIGMA2 | TRAIN_S, R)) return rc;
  MissingFront F;
  if (int rc = missing_front(R.yd.p, n, p, U, S, m, sigma2, R.means.data(), latent_begin, latent_end, false, F)) return rc;
  std::vector<double> lml;
  if (int rc = latent_lmls(R.xd.p, d, n, R.lts, nullptr, latent_begin, latent_end, F.z.p, lml, 1, F.nv.p)) return rc;
  double total = 0.0;
  for (double v : lml) total += v;
  if (with_regulariser) total += F.reg(n, m, sigma2);
  *out = total;
  return LMM_OK;
  LMM_CATCH
}

int lmm_oilmm_posterior_create_missing(const double* x, int d, int n, const double* y, int p, const double* U, const double* S, int m,
                                       double sigma2, const lmm_gp_t* gps, int latent_begin, int latent_end, lmm_post_t** out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  Train R;
  if (int rc = train(!x || !y || !U || !S || !out || d <= 0 || n <= 0 || p <= 0 || m <= 0, x, d, n, y, (size_t)n * p, p, S, m, sigma2, gps, latent_begin,
                     latent_end, TRAIN_SIGMA2 | TRAIN_S, R)) return rc;
  MissingFront F;
  if (int rc = missing_front(R.yd.p, n, p, U, S, m, sigma2, R.means.data(), latent_begin, latent_end, false, F)) return rc;
  return posterior_create_common(R.xd.p, d, n, R.ls, nullptr, latent_begin, latent_end, F.z.p, out, F.nv.p);
  LMM_CATCH
}

// The back end of the OILMM gradients for data with NaN (oilmm_grad_missing_core, ss_logpdf_grad), over the n points the front end F
// numbered: the regulariser's share of d/dsigma2 (added to G.gs2[0]) and d/dY through the per-point projections (gy_dev: n x p, device,
// or nullptr) from a = -d value / d r (device, latent k of the shard at a + k lda).  The latents' share of d/dsigma2 stays with the paths.
static void missing_grad_back_end(const MissingFront& F, int n, int p, int m, double s2, int with_regulariser, const double* a, int lda,
                                  int l0, int ms, OilmmGrad& G, double* gy_dev) {
  if (with_regulariser) G.gs2[0] += -0.5 * ((F.sum_pt - (double)n * m) / s2 - F.rss / (s2 * s2));
  if (gy_dev)
    launch_missing_grad_y(n, p, m, F.pat_of.p, F.pmask.p, F.Tpat.p, a, lda, l0, ms, with_regulariser ? F.resid.p : nullptr, s2, gy_dev,
                          g.streams[0]);
}

// The path beside oilmm_grad_core for precomputed per-latent residuals and per-point noise (F.z, F.nv): the same per-latent factor,
// alpha, Kt^-1 and launch_grad_reduce; the chain rule runs through the per-point noise (missing_wdiag_kernel) instead of s2 / S, and
// d/dy through the per-point projection (missing_grad_y_kernel).  No derivatives with respect to S, U or x.
static int oilmm_grad_missing_core(const double* xd, int d, int n, int p, double s2, const LatentSet* ls, int l0, int l1,
                                   int with_regulariser, const MissingFront& F, OilmmGrad& G, double* gy_dev) {
  hipStream_t st0 = g.streams[0];
  const int m = (int)ls->lat.size(), ms = l1 - l0;
  KernelGradPass K(ls, l0, l1, n, d);
  Buf<double> wd(2 * (size_t)K.F.mk);        // alpha' D alpha and tr(Kt^-1 D) per latent, D its per-point noise
  K.launch(xd, F.z.p, nullptr, F.nv.p, n, [](const FanBatch&, int, const double*, const double*, const LatentDev&) {},
           [&](const FanBatch& b, int k, const double* Kinv, const double* al) {
             launch_missing_wdiag(Kinv, K.D.ld, n, al, F.nv.p + (size_t)k * n, wd.p + 2 * (size_t)k, b.st);
           });
  K.read_back();
  std::vector<double> hwd(2 * (size_t)K.F.mk, 0.0);
  if (ms > 0) HIPCHK(hipMemcpyAsync(hwd.data(), wd.p, hwd.size() * sizeof(double), hipMemcpyDeviceToHost, st0));
  K.F.fetch_info();
  G.size(m, p, 1, d);
  missing_grad_back_end(F, n, p, m, s2, with_regulariser, K.alpha.p, K.D.NC, l0, ms, G, gy_dev);      // d/dY is queued ahead of the wait for the pivots
  if (int rc = K.F.check(l0)) return rc;
  double total = 0.0, gs2 = 0.0;
  for (int k = 0; k < ms; ++k) {
    total += K.lml[k];
    const double* r = K.sums(k);
    const double D_aa = hwd[2 * (size_t)k], D_tr = hwd[2 * (size_t)k + 1];      // alpha' D alpha, tr(Kt^-1 D), D = diag(s2 (G_t^-1)_ll)
    K.finish(k, D_aa, D_tr, r[2], r[1], G.ggps, G.trec);
    gs2 += 0.5 * (D_aa - D_tr) / s2;            // sum_t c_lt (alpha_t^2 - (Kt^-1)_tt) / 2, c_lt = (G_t^-1)_ll
  }
  if (with_regulariser) total += F.reg(n, m, s2);
  G.value = total;
  G.gs2[0] += gs2;                              // (the latents' sum + the regulariser's term: addition commutes)
  return LMM_OK;
}

int lmm_oilmm_logpdf_grad_missing(const double* x, int d, int n, const double* y, int p, const double* U, const double* S, int m,
                                  double sigma2, const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser,
                                  double* out_logpdf, double* grad_y, double* grad_sigma2, lmm_gp_grad_t* grad_gps) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  Train R;
  if (int rc = train(!x || !y || !U || !S || !out_logpdf || d <= 0 || n <= 0 || p <= 0 || m <= 0, x, d, n, y, (size_t)n * p, p, S, m, sigma2, gps, latent_begin,
                     latent_end, TRAIN_SIGMA2 | TRAIN_S, R)) return rc;
  if (int rc = R.ls->ard_grad_check()) return rc;
  hipStream_t st0 = g.streams[0];
  DevOut gy(grad_y, (size_t)n * p);
  MissingFront F;
  if (int rc = missing_front(R.yd.p, n, p, U, S, m, sigma2, R.means.data(), latent_begin, latent_end, grad_y && with_regulariser, F)) return rc;
  OilmmGrad G;
  if (int rc = oilmm_grad_missing_core(R.xd.p, d, n, p, sigma2, R.ls.get(), latent_begin, latent_end, with_regulariser, F, G, gy.p)) return rc;
  write_oilmm_grad(G, out_logpdf, grad_sigma2, nullptr, nullptr, grad_gps);
  publish_grads(*R.ls, grad_gps ? &G.trec : nullptr, latent_begin, latent_end);
  if (grad_y) { gy.finish(st0); HIPCHK(hipStreamSynchronize(st0)); }
  return LMM_OK;
  LMM_CATCH
}

int lmm_mogp_posterior_create(const double* x, int d, int n, const double* y, int m, double sigma2, const lmm_gp_t* gps,
                              int latent_begin, int latent_end, lmm_post_t** out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  Train R;
  if (int rc = train(!x || !y || !out || d <= 0 || n <= 0 || m <= 0, x, d, n, y, (size_t)n * m, m, nullptr, m, sigma2, gps, latent_begin, latent_end, 0, R))
    return rc;
  OilmmFront F = OilmmFront::identity(m);
  F.upload(R.means);
  Buf<double> delta = F.delta(R.yd.p, n, R.l0, R.ms);
  const std::vector<double> noise(m, sigma2);
  return posterior_create_common(R.xd.p, d, n, R.ls, noise.data(), latent_begin, latent_end, delta.p, out);
  LMM_CATCH
}

// Dense-H posterior state from the stacked inputs xd (d x n, device), the projected residuals delta ([latent][point], m n,
// device) and the per-batch SigmaT list: assemble blockdiag(K_l) + SigmaT_{batch(i)} (x) e_i e_i', factor, alpha = C \ delta.
static int dense_posterior_build(const double* xd, int d, int n, const double* H, int p, std::shared_ptr<LatentSet> ls,
                                 const double* delta, const std::vector<double>& sigs, const std::vector<int>& sigidx,
                                 lmm_post_t** out) {
  const int m = (int)ls->lat.size();
  const Latent* lts = ls->lat.data();
  if ((long long)m * n > 2000000000LL / 64) return fail(LMM_ERR_UNSUPPORTED, "m*n too large for the dense path");
  hipStream_t st0 = g.streams[0];
  std::vector<LatentDev> lat(m);
  for (int l = 0; l < m; ++l) lat[l] = lts[l].dense_dev();
  const int N = m * n;
  Dims D(N, 1);
  lmm_post* P = new lmm_post();
  try {
    P->kind = 1; P->f32 = g_f32; P->n = n; P->d = d; P->l0 = 0; P->l1 = m; P->m = m; P->p = p;
    P->NC = D.NC; P->NR = D.NR; P->ld = D.ld;
    P->ls = std::move(ls);
    P->H.assign(H, H + (size_t)p * m);
    P->sigs = sigs; P->sigidx = sigidx;
    P->x = Buf<double>((size_t)d * n);
    HIPCHK(hipMemcpyAsync(P->x.p, xd, (size_t)d * n * sizeof(double), hipMemcpyDeviceToDevice, st0));
    P->latd = Buf<LatentDev>(m);
    HIPCHK(hipMemcpyAsync(P->latd.p, lat.data(), m * sizeof(LatentDev), hipMemcpyHostToDevice, st0));
    P->ddelta = Buf<double>((size_t)N);
    HIPCHK(hipMemcpyAsync(P->ddelta.p, delta, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, st0));
    Uploaded STd(sigs, st0);
    Buf<int> idxd(n);
    HIPCHK(hipMemcpyAsync(idxd.p, sigidx.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st0));
    P->L.emplace_back(mat_count(D.elems()));
    P->W.emplace_back(mat_count((size_t)(D.NC / 64) * 4096));
    P->alpha.emplace_back((size_t)D.NC);
    P->z.emplace_back((size_t)D.NC);          // z = L^-1 delta (the rider row): the fp32 mode's means are mu + R' z, not mu + K(x*, x) alpha
    DenseFactor C(N, 1, st0, P->L[0].p, P->W[0].p);      // the handle keeps the factor
    dense_assemble(C.A, D, P->x.p, d, n, m, P->latd.p, P->ls->any_sum(), STd.buf.p, idxd.p, P->ddelta.p, 1, st0);
    C.factor(false, st0);
    HIPCHK(hipMemsetAsync(P->alpha[0].p, 0, (size_t)D.NC * sizeof(double), st0));
    launch_extract_row(C.A, D.ld, D.NC, N, P->alpha[0].p, st0);
    HIPCHK(hipMemcpyAsync(P->z[0].p, P->alpha[0].p, (size_t)D.NC * sizeof(double), hipMemcpyDeviceToDevice, st0));
    backsolve1(C.A, D.ld, C.W, D.NC / 64, P->alpha[0].p, st0);
    if (int rc = C.finish(nullptr, st0)) { delete P; return rc; }
  } catch (int code) { drain_after_error(); delete P; return code; }
  *out = P;
  return LMM_OK;
}

// posterior(fx::FiniteGP{<:ILMM}, y), dense H: reference src/ilmm.jl:184-198.  One (mn) x (mn) factorisation kept on the
// device with alpha = C \ (Yproj - mean).
int lmm_ilmm_posterior_create(const double* x, int d, int n, const double* y, int p, const double* H, int m, double sigma2,
                              const lmm_gp_t* gps, const lmm_jitters_t* jit, lmm_post_t** out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!x || !y || !H || !out || d <= 0 || n <= 0 || p <= 0 || m <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  RESOLVE(gps, m, d);
  if (!jit) jit = &kDefaultJit;
  hipStream_t st0 = g.streams[0];
  DenseFront F(H, p, m);
  if (int rc = F.project(sigma2, jit->project_jitter, false)) return rc;
  DevIn xd(x, (size_t)d * n, st0), yd(y, (size_t)n * p, st0);
  F.upload(lts, 0);
  Buf<double> delta((size_t)n * m);
  F.delta(yd.p, n, delta.p);
  return dense_posterior_build(xd.p, d, n, H, p, ls, delta.p, F.ST, std::vector<int>(n, 0), out);
  LMM_CATCH
}

// posterior(pi(x2, sigma2), y2) on the dense-H posterior ILMM (AbstractGPs.TestUtils on `pi`, reference test/ilmm.jl:34-37;
// src/ilmm.jl:184-198 applied to the PosteriorGP latent): the posterior of the PRIOR given both projected data sets, each
// with its own SigmaT (x) I noise.  Returns a NEW handle.
int lmm_ilmm_post_condition(const lmm_post_t* post, double sigma2, const double* x2, int d, int n2, const double* y2,
                            const lmm_jitters_t* jit, lmm_post_t** out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  const lmm_post* P = post;
  const lmm_post* D = nullptr;
  if (int rc = dense_post_args(post, !x2 || !y2 || !out || d <= 0 || n2 <= 0, d, D, jit)) return rc;
  hipStream_t st0 = g.streams[0];
  const int m = P->m, p = P->p, n1 = P->n, n = n1 + n2;
  DenseFront F(P->H.data(), p, m);
  if (int rc = F.project(sigma2, jit->project_jitter, false)) return rc;
  DevIn x2d(x2, (size_t)d * n2, st0), y2d(y2, (size_t)n2 * p, st0);
  F.upload(P->ls->lat.data(), 0);
  Buf<double> d2((size_t)n2 * m), delta((size_t)n * m), xall((size_t)d * n);
  F.delta(y2d.p, n2, d2.p);
  HIPCHK(hipMemcpyAsync(xall.p, D->x.p, (size_t)d * n1 * sizeof(double), hipMemcpyDeviceToDevice, st0));
  HIPCHK(hipMemcpyAsync(xall.p + (size_t)d * n1, x2d.p, (size_t)d * n2 * sizeof(double), hipMemcpyDeviceToDevice, st0));
  for (int l = 0; l < m; ++l) {
    HIPCHK(hipMemcpyAsync(delta.p + (size_t)l * n, D->ddelta.p + (size_t)l * n1, (size_t)n1 * sizeof(double), hipMemcpyDeviceToDevice, st0));
    HIPCHK(hipMemcpyAsync(delta.p + (size_t)l * n + n1, d2.p + (size_t)l * n2, (size_t)n2 * sizeof(double), hipMemcpyDeviceToDevice, st0));
  }
  std::vector<double> sigs = P->sigs;
  sigs.insert(sigs.end(), F.ST.begin(), F.ST.end());
  std::vector<int> idx = P->sigidx;
  idx.resize(n, (int)(P->sigs.size() / ((size_t)m * m)));
  return dense_posterior_build(xall.p, d, n, P->H.data(), p, P->ls, delta.p, sigs, idx, out);
  LMM_CATCH
}

static void dense_post_cross(const lmm_post* P, const double* xsd, int d, int ns, int nr, double* R, int ldr, hipStream_t st);
static void dense_post_means(const lmm_post* P, const double* xsd, int d, int ns, const double* R, int ldr, double* ml, hipStream_t st);

int lmm_ilmm_post_mean_and_var(const lmm_post_t* post, double sigma2, const double* xs, int d, int ns,
                               const lmm_jitters_t* jit, double* mean_out, double* var_out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  const lmm_post* P = post;
  const lmm_post* D = nullptr;
  if (int rc = dense_post_args(post, !xs || !mean_out || !var_out || d <= 0 || ns <= 0, d, D, jit)) return rc;
  hipStream_t st0 = g.streams[0];
  const int m = P->m, p = P->p, n = P->n, N = m * n;
  DevIn xsd(xs, (size_t)d * ns, st0);
  Uploaded Hd(P->H, st0);
  Buf<double> ml((size_t)ns * m);
  const int nr = rup(m * ns, 64);
  const int ldr = pad_ld(nr);
  Buf<double> R(mat_count((size_t)ldr * P->NC));
  dense_post_cross(P, xsd.p, d, ns, nr, R.p, ldr, st0);
  dense_post_means(P, xsd.p, d, ns, R.p, ldr, ml.p, st0);
  DevOut mo(mean_out, (size_t)ns * p), vo(var_out, (size_t)ns * p);
  launch_mix(ml.p, ns, m, Hd.buf.p, p, 1, 0.0, 0.0, nullptr, 0.0, mo.p, st0);
  Buf<double> dv_part(dense_var_partial_elems(ns, p, N));
  launch_dense_var(R.p, ldr, ns, m, N, Hd.buf.p, p, D->latd.p, jit->default_jitter, sigma2, dv_part.p, vo.p, st0);
  mo.finish(st0); vo.finish(st0);
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

// Dense-H posterior: R (nr x NC, ldr; rows (l, s) = l ns + s, rows >= m ns zero) = K(xs, x)' L^-T.  Caller holds g_mu.
static void dense_post_cross(const lmm_post* P, const double* xsd, int d, int ns, int nr, double* R, int ldr, hipStream_t st) {
  const lmm_post* D = dense_state(P);
  guard_extent(R, nr, ldr, P->NC, true, "dense-H cross-Gram");
  launch_dense_cross(R, ldr, nr, P->NC, xsd, ns, D->x.p, P->n, d, P->m, D->latd.p, D->ls->any_sum(), st);
  trsm_rec(R, ldr, nr, D->L[0].p, P->ld, D->W[0].p, 0, P->NC, st);
}
// Latent posterior means at xs, ml[l ns + s].  Float64: mu_l + K(x*, x) alpha_l (no solve needed).  fp32 compute mode: that sum cancels
// over weights alpha = Kt^-1 delta whose Float32-factor error is amplified by cond |alpha| (section 4.3 of DESIGN.md: 0.15 absolute at
// n = 1100 on the per-latent path), so the means take the rider form mu_l + R (L^-1 delta) from the cross-solve block R (which the
// caller has computed: dense_post_cross; rows >= m ns of R are zero).
static void dense_post_means(const lmm_post* P, const double* xsd, int d, int ns, const double* R, int ldr, double* ml, hipStream_t st) {
  const lmm_post* D = dense_state(P);
  const int m = P->m, n = P->n;
  if (!g_f32) {
    Buf<double> pm_part(post_mean_partial_elems(ns, n));
    for (int l = 0; l < m; ++l)
      post_mean_g(xsd, ns, D->x.p, n, d, D->alpha[0].p + (size_t)l * n, P->ls->lat[l], pm_part.p, ml + (size_t)l * ns, st);
    HIPCHK(hipStreamSynchronize(st));              // pm_part is released on return
    return;
  }
  Buf<double> part(strip_partial_elems(m * ns, m * n, 1)), mu((size_t)m * ns);
  rider_stats_g(R, ldr, m * ns, m * n, D->z[0].p, 0.0, 0.0, part.p, ml, nullptr, st);
  for (int l = 0; l < m; ++l) launch_fill(mu.p + (size_t)l * ns, ns, P->ls->lat[l].mean, st);
  launch_vec_lin(ml, mu.p, 1.0, m * ns, ml, st);
  HIPCHK(hipStreamSynchronize(st));
}
// Latent joint covariance at xs as a factor matrix,  blockdiag(K_l(xs,xs)) + SigAdd (x) I_ns - R R'  (R from dense_post_cross with
// nr = Ds.NC rows), optional rider row; a caller that wants its Cholesky gives the A of a DenseFactor and factors that.
static void dense_post_cov_factor(const lmm_post* P, const double* xsd, int d, int ns, const double* sigadd_dev,
                                  const double* rider, const Dims& Ds, double* A, const double* R, int ldr, hipStream_t st) {
  const lmm_post* D = dense_state(P);
  guard_extent(A, Ds.NR, Ds.ld, Ds.NC, true, "dense-H posterior covariance");
  dense_assemble(A, Ds, xsd, d, ns, P->m, D->latd.p, D->ls->any_sum(), sigadd_dev, nullptr, rider, rider ? 1 : 0, st);
  gemm_nt_g(A, Ds.ld, R, ldr, R, ldr, Ds.NC, Ds.NC, P->NC, 1, false, st, "Schur complement (dense-H posterior covariance)");
}

// mean_and_cov(pi(xs, sigma2)) / cov on the dense-H posterior ILMM (reference src/ilmm.jl:132-147 with the PosteriorGP latent
// of :196-197; AbstractGPs.TestUtils secondary interface on `pi`, test/ilmm.jl:34-37): C = H_full (Cov_latent + 1e-18 I)
// H_full' + sigma2 I, (p ns) x (p ns) column-major, by-outputs order.
int lmm_ilmm_post_mean_and_cov(const lmm_post_t* post, double sigma2, const double* xs, int d, int ns,
                               const lmm_jitters_t* jit, double* mean_out, double* cov_out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  const lmm_post* P = post;
  const lmm_post* D = nullptr;
  if (int rc = dense_post_args(post, !xs || !mean_out || !cov_out || d <= 0 || ns <= 0, d, D, jit)) return rc;
  const int m = P->m, p = P->p, Ns = m * ns;
  if ((double)p * ns * (double)p * ns > 4e8) return fail(LMM_ERR_UNSUPPORTED, "full covariance (p*ns)^2 too large");
  hipStream_t st0 = g.streams[0];
  DevIn xsd(xs, (size_t)d * ns, st0);
  Uploaded Hd(P->H, st0), Zd(std::vector<double>((size_t)m * m, 0.0), st0);
  Buf<double> ml((size_t)Ns);
  Dims Ds(Ns, 0);
  const int ldr = pad_ld(Ds.NC);
  Buf<double> A(mat_count(Ds.elems())), R(mat_count((size_t)ldr * P->NC)), T((size_t)p * ns * Ns);
  dense_post_cross(P, xsd.p, d, ns, Ds.NC, R.p, ldr, st0);
  dense_post_means(P, xsd.p, d, ns, R.p, ldr, ml.p, st0);
  dense_post_cov_factor(P, xsd.p, d, ns, Zd.buf.p, nullptr, Ds, A.p, R.p, ldr, st0);
  DevOut mo(mean_out, (size_t)ns * p), co(cov_out, (size_t)ns * p * ns * p);
  launch_mix(ml.p, ns, m, Hd.buf.p, p, 1, 0.0, 0.0, nullptr, 0.0, mo.p, st0);
  launch_dense_cov(A.p, Ds.ld, ns, m, Hd.buf.p, p, jit->default_jitter, sigma2, T.p, co.p, st0);
  mo.finish(st0); co.finish(st0);
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

// logpdf(pi(xs, sigma2), ys) on the dense-H posterior ILMM (reference test/ilmm.jl:25; src/ilmm.jl:150-163 with the
// PosteriorGP latent of :196-197): project ys, one (m ns) x (m ns) factorisation of latent posterior cov + SigmaT (x) I.
int lmm_ilmm_post_logpdf(const lmm_post_t* post, double sigma2, const double* xs, int d, int ns, const double* ys,
                         const lmm_jitters_t* jit, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  const lmm_post* P = post;
  const lmm_post* D = nullptr;
  if (int rc = dense_post_args(post, !xs || !ys || !out || d <= 0 || ns <= 0, d, D, jit)) return rc;
  hipStream_t st0 = g.streams[0];
  const int m = P->m, p = P->p, Ns = m * ns;
  DenseFront F(P->H.data(), p, m);
  if (int rc = F.project(sigma2, jit->project_jitter, true)) return rc;
  DevIn xsd(xs, (size_t)d * ns, st0), ysd(ys, (size_t)ns * p, st0);
  F.upload(nullptr, ns);                           // (the handle has the latents; their posterior means come below)
  Buf<double> ml((size_t)ns * m), delta((size_t)ns * m), resid_dev(1);
  F.residual(ysd.p, ns, resid_dev.p);
  const Dims Ds(Ns, 1);
  const int ldr = pad_ld(Ds.NC);
  Buf<double> R(mat_count((size_t)ldr * P->NC));
  dense_post_cross(P, xsd.p, d, ns, Ds.NC, R.p, ldr, st0);
  dense_post_means(P, xsd.p, d, ns, R.p, ldr, ml.p, st0);
  launch_vec_lin(F.Ty.p, ml.p, -1.0, Ns, delta.p, st0);
  DenseFactor C(Ns, 1, st0);
  dense_post_cov_factor(P, xsd.p, d, ns, F.STd.buf.p, delta.p, C.D, C.A, R.p, ldr, st0);
  C.factor(true, st0);
  double lml = 0.0, resid = 0.0;
  HIPCHK(hipMemcpyAsync(&resid, resid_dev.p, sizeof(double), hipMemcpyDeviceToHost, st0));
  if (int rc = C.finish(&lml, st0)) return rc;
  *out = lml + ilmm_regulariser(ns, p, m, sigma2, F.logdetST, resid);
  return LMM_OK;
  LMM_CATCH
}

// rand(rng, pi(xs, sigma2)) on the dense-H posterior ILMM (reference src/ilmm.jl:78-87 with the PosteriorGP latent): the
// latent joint sample mean + chol(Cov + 1e-12 I).U' z  (z: m*ns normals), mixed by H, plus sqrt(sigma2) eps.
int lmm_ilmm_post_rand(const lmm_post_t* post, double sigma2, int add_noise, const double* xs, int d, int ns,
                       const double* z_lat, const double* eps, const lmm_jitters_t* jit, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  const lmm_post* P = post;
  const lmm_post* D = nullptr;
  if (int rc = dense_post_args(post, !xs || !z_lat || !out || d <= 0 || ns <= 0 || (add_noise && !eps), d, D, jit)) return rc;
  hipStream_t st0 = g.streams[0];
  const int m = P->m, p = P->p, Ns = m * ns;
  std::vector<double> J((size_t)m * m, 0.0);
  for (int l = 0; l < m; ++l) J[l + (size_t)l * m] = jit->ilmm_rand_jitter;
  DevIn xsd(xs, (size_t)d * ns, st0), zd(z_lat, (size_t)Ns, st0), epsd(add_noise ? eps : nullptr, (size_t)ns * p, st0);
  Uploaded Jd(J, st0), Hd(P->H, st0);
  Buf<double> ml((size_t)Ns), X((size_t)Ns);
  const Dims Ds(Ns, 0);
  const int ldr = pad_ld(Ds.NC);
  Buf<double> R(mat_count((size_t)ldr * P->NC)), part(strip_partial_elems(Ns, Ns, 1));
  dense_post_cross(P, xsd.p, d, ns, Ds.NC, R.p, ldr, st0);
  dense_post_means(P, xsd.p, d, ns, R.p, ldr, ml.p, st0);
  DenseFactor C(Ns, 0, st0);
  dense_post_cov_factor(P, xsd.p, d, ns, Jd.buf.p, nullptr, C.D, C.A, R.p, ldr, st0);
  C.factor(false, st0);
  launch_trmv_lower(C.A, C.D.ld, Ns, zd.p, 0.0, part.p, X.p, st0);
  launch_vec_lin(X.p, ml.p, 1.0, Ns, X.p, st0);
  DevOut od(out, (size_t)ns * p);
  launch_mix(X.p, ns, m, Hd.buf.p, p, 1, 0.0, 0.0, add_noise ? epsd.p : nullptr, std::sqrt(sigma2), od.p, st0);
  od.finish(st0);
  return C.finish(nullptr, st0);
  LMM_CATCH
}

// get_latent_gp(posterior(fx::FiniteGP{<:ILMM}, y)) for a dense H (reference src/ilmm.jl:39 on the ILMM of :196-197): the latent
// PosteriorGP{IndependentMOGP} as a handle of its own.  It SHARES the device state of `post` (the (mn) x (mn) factor, alpha, x)
// and differs only in H = I_m, p = m, so every lmm_ilmm_post_* entry point answers for the m latent outputs at
// MOInputIsotopicByOutputs(xs, m): with project_jitter = 0 the projection is the identity, SigmaT = sigma2 I and the regulariser
// vanishes, i.e. logpdf is the generic Gaussian of the latent posterior + sigma2 I; rand with ilmm_rand_jitter = sigma2 and
// add_noise = 0 is AbstractGPs' mean + chol(cov + sigma2 I).U' z.  Destroy it with lmm_post_destroy (either order w.r.t. `post`).
int lmm_ilmm_post_latent_view(const lmm_post_t* post, lmm_post_t** out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!post || !out) return fail(LMM_ERR_ARG, "bad arguments");
  if (post->kind != 1) return fail(LMM_ERR_ARG, "not a dense-H ILMM posterior");
  lmm_post* B = const_cast<lmm_post*>(dense_state(post));
  lmm_post* V = new lmm_post();
  V->f32 = B->f32; V->kind = 1; V->n = B->n; V->d = B->d; V->l0 = 0; V->l1 = B->m; V->m = B->m; V->p = B->m;
  V->NC = B->NC; V->NR = B->NR; V->ld = B->ld;
  V->ls = B->ls; V->sigs = B->sigs; V->sigidx = B->sigidx;
  V->H.assign((size_t)B->m * B->m, 0.0);
  for (int l = 0; l < B->m; ++l) V->H[l + (size_t)l * B->m] = 1.0;
  V->base = B;
  ++B->views;
  *out = V;
  return LMM_OK;
  LMM_CATCH
}

int lmm_post_destroy(lmm_post_t* post) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (post) {
    if (g.init) (void)hipDeviceSynchronize();
    if (post->base) {                                   // a latent view: release the base if it was waiting for its last view
      lmm_post* B = post->base;
      if (--B->views == 0 && B->zombie) delete B;
      delete post;
    } else if (post->views > 0) {
      post->zombie = true;                              // views still use this state: freed with the last of them
    } else {
      delete post;
    }
  }
  return LMM_OK;
}

// Rk (nsr x NC, ldr) = K(xs, x): the cross-Gram of a posterior latent's training inputs as rider rows (rows beyond ns zero).
static GramArgs cross_gram_args(const lmm_post* P, const Latent& gp, const double* xsd, int d, int ns, double* Rk, int ldr,
                                int nsr) {
  GramArgs r{};
  r.A = Rk; r.ld = ldr; r.nrows = P->NC + nsr; r.ncols = P->NC; r.row_tile0 = P->NC / 64; r.row_shift = P->NC; r.full = 1;
  r.x = P->x.p; r.d = d; r.n = P->n; gp.set_kernel(r);
  r.xs = xsd; r.ns = ns;
  return r;
}
static void cross_gram(const lmm_post* P, const Latent& gp, const double* xsd, int d, int ns, double* Rk, int ldr, int nsr,
                       hipStream_t st) {
  gram_g(cross_gram_args(P, gp, xsd, d, ns, Rk, ldr, nsr), st);
}

// The cross-solve blocks of a fan-out over a posterior's latents: per slot nb_per buffers R (nsr x P->NC, ldr), and for a batch
// R_j <- K(xs, x) L_j^-T of its latents -- one batched cross-Gram launch (rows beyond ns zero), one batched triangular solve.
struct CrossSlots {
  int nsr, ldr;
  std::vector<std::vector<Buf<double>>> R;
  BatchPtr Rb{}, Lb{}, Wb{};       // the operands of the batch solved last (for what a caller runs on them next)
  explicit CrossSlots(int nsr_) : nsr(nsr_), ldr(pad_ld(nsr_)) {}
  double elems(const lmm_post* P) const { return (double)ldr * P->NC; }
  void alloc(const lmm_post* P, const FanOut& F) {
    R.resize(F.nslots);
    for (int s = 0; s < F.nslots; ++s)
      for (int j = 0; j < F.nb_per; ++j) R[s].emplace_back(mat_count((size_t)ldr * P->NC));
  }
  // det: no split-K in the solve's updates; prof: the Gram launch is one ProfScope of the cross-Gram's n* x n rectangle
  void solve(const lmm_post* P, const FanBatch& b, const double* xsd, int d, int ns, bool det, bool prof) {
    GramArgs ga[LMM_MAX_BATCH];
    for (int j = 0; j < b.nb; ++j) {
      const int k = b.k0 + j;
      ga[j] = cross_gram_args(P, P->ls->lat[P->l0 + k], xsd, d, ns, R[b.s][j].p, ldr, nsr);
      Rb.p[j] = R[b.s][j].p; Lb.p[j] = P->L[k].p; Wb.p[j] = P->W[k].p;
    }
    if (prof) {
      const double gb = (double)ns * P->n * 8.0;                   // cross-Gram K(x*, x): a full n* x n rectangle written once
      ProfScope ps(LMM_PROF_GRAM, b.nb * gb, b.st, 0, 0, 0, b.nb * gb, b.nb);
      gram_batch_g(ga, b.nb, b.st);
    } else gram_batch_g(ga, b.nb, b.st);
    trsm_rec(Rb, ldr, nsr, Lb, P->ld, Wb, b.nb, 0, P->NC, b.st, false, true, det);       // R_j <- K(x*, x) L_j^-T for the whole batch
  }
};

// Latent marginals (mean, var) of latents [l0, l1) at xs into device arrays (ns per latent).
// post != NULL: posterior latents; else the prior latents lts_shard[0..ms).  Caller holds g_mu.
static int latent_marginals_dev(const lmm_post* P, const Latent* lts_shard, int ms, const double* xsd, int d, int ns,
                                double* mean_lat, double* var_lat) {
  if (ms == 0) return LMM_OK;
  if (P == nullptr) {
    for (int k = 0; k < ms; ++k) {
      // prior: constant mean, variance kappa(0)
      rider_stats_g(nullptr, 0, ns, 0, nullptr, lts_shard[k].mean, lts_shard[k].prior_var(), nullptr, mean_lat + (size_t)k * ns,
                         var_lat + (size_t)k * ns, g.streams[0]);
    }
    return LMM_OK;
  }
  if (P->d != d) return fail(LMM_ERR_DIM, "input dimension mismatch: posterior has d=%d, xs has d=%d", P->d, d);
  CrossSlots C(rup(ns, 64));
  FanOut F(ms, mat_bytes(C.elems(P)));
  C.alloc(P, F);
  std::vector<Buf<double>> part;
  for (int s = 0; s < F.nslots; ++s) part.emplace_back(strip_partial_elems(C.nsr, P->NC, 2));
  F.run([&](const FanBatch& b) {
    C.solve(P, b, xsd, d, ns, false, true);
    for (int j = 0; j < b.nb; ++j) {
      const int k = b.k0 + j;
      const Latent& gp = P->ls->lat[P->l0 + k];
      // mean = mu + K(x*,x) alpha = mu + R' (L^-1 delta);  var = kappa(0) - colsumsq(R)   (one pass over R)
      const double rb = (double)ns * P->n * 8.0;                   // R read once
      ProfScope ps(LMM_PROF_STRIP, rb, b.st, ns, P->n, 0, rb);
      rider_stats_g(C.R[b.s][j].p, C.ldr, ns, P->n, P->z[k].p, gp.mean, gp.prior_var(), part[b.s].p, mean_lat + (size_t)k * ns,
                         var_lat + (size_t)k * ns, b.st);
    }
  });
  HIPCHK(hipStreamSynchronize(g.streams[0]));   // R buffers are released on return
  return LMM_OK;
}

int lmm_latent_marginals(const lmm_post_t* post, const lmm_gp_t* gps, int m_shard, const double* xs, int d, int ns,
                         double* mean_lat, double* var_lat) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (int rc = post_dtype_check(post)) return rc;
  if (!xs || !mean_lat || !var_lat || d <= 0 || ns <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  if (post && post->kind != 0) return fail(LMM_ERR_UNSUPPORTED, "per-latent marginals of the dense-H posterior (coupled latents): use lmm_ilmm_post_mean_and_var");
  const int ms = post ? (post->l1 - post->l0) : m_shard;
  std::shared_ptr<LatentSet> ls;
  if (!post) { if (int rc = resolve(gps, m_shard, d, ls)) return rc; }
  hipStream_t st0 = g.streams[0];
  DevIn xsd(xs, (size_t)d * ns, st0);
  DevOut mo(mean_lat, (size_t)ns * ms), vo(var_lat, (size_t)ns * ms);
  if (int rc = latent_marginals_dev(post, post ? nullptr : ls->lat.data(), ms, xsd.p, d, ns, mo.p, vo.p)) return rc;
  mo.finish(st0); vo.finish(st0);
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

int lmm_oilmm_mean_and_var(const lmm_post_t* post, const lmm_gp_t* gps, const double* U, const double* S, int p, int m,
                           int latent_begin, int latent_end, double sigma2, int add_noise, const double* xs, int d,
                           int ns, const lmm_jitters_t* jit, double* mean_out, double* var_out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (int rc = post_dtype_check(post)) return rc;
  if (!U || !xs || !mean_out || d <= 0 || ns <= 0 || p <= 0 || m <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  if (!jit) jit = &kDefaultJit;
  Shard Q;      // (d is checked on the mean-only path below, and by the cross solve)
  if (int rc = post_shard(post, "dense-H posterior handle: use lmm_ilmm_post_mean_and_var", gps, m, d, latent_begin, latent_end, Q, nullptr)) return rc;
  if (int rc = shard_check(Q.l0, Q.l1, m)) return rc;
  const Latent* lts = Q.lts;
  const int l0 = Q.l0, ms = Q.ms;
  hipStream_t st0 = g.streams[0];
  const std::vector<double> Hs = shard_H(U, S, p, l0, ms);      // H columns of the shard (p x ms)
  Uploaded Hd(Hs, st0);
  DevIn xsd(xs, (size_t)d * ns, st0);
  Buf<double> ml((size_t)ns * std::max(ms, 1)), vl((size_t)ns * std::max(ms, 1));
  // fp32 mode: mu + K(x*, x) alpha is a cancelling sum over weights alpha = Kt^-1 delta whose Float32-factor error is amplified
  // (cond x eps x |alpha|); the rider form mu + R' (L^-1 delta) of the full path is stable, so posterior means take that path
  const bool mean_only = var_out == nullptr && !(g_f32 && post);
  if (mean_only) {
    // mean only (AbstractGPs.mean(fx), reference src/ilmm.jl:142 -> mean_and_var(fx)[1]): the posterior latent means are
    // mu + K(x*, x) alpha -- n n* kernel evaluations, no triangular solve (the reference pays for the variances it discards)
    if (post && post->d != d) return fail(LMM_ERR_DIM, "input dimension mismatch: posterior has d=%d, xs has d=%d", post->d, d);
    Buf<double> pm_part(post ? post_mean_partial_elems(ns, post->n) : 1);
    for (int k = 0; k < ms; ++k) {
      const Latent& gp = lts[l0 + k];
      post_mean_g(xsd.p, ns, post ? post->x.p : nullptr, post ? post->n : 0, d, post ? post->alpha[k].p : nullptr, gp,
                  pm_part.p, ml.p + (size_t)k * ns, st0);
    }
    DevOut mo(mean_out, (size_t)ns * p);
    mix_marginals(ml.p, ns, ms, Hd.buf.p, p, 1, 0.0, 0.0, mo.p, st0);
    mo.finish(st0);
    HIPCHK(hipStreamSynchronize(st0));
    return LMM_OK;
  }
  if (int rc = latent_marginals_dev(post, post ? nullptr : lts + l0, ms, xsd.p, d, ns, ml.p, vl.p)) return rc;
  DevOut mo(mean_out, (size_t)ns * p), vo(var_out, (size_t)ns * p);
  // reference src/oilmm.jl:69,72: M = H M_latent;  V = abs2.(H) V_latent .+ sigma2   (V_latent carries the 1e-18 jitter);
  // Float64 VALU by default, v_mfma_f32_16x16x32_bf16 under lmm_set_projection_dtype(LMM_PROJ_BF16 / _BF16X2)
  mix_marginals(ml.p, ns, ms, Hd.buf.p, p, 1, 0.0, 0.0, mo.p, st0);
  if (var_out) mix_marginals(vl.p, ns, ms, Hd.buf.p, p, 2, jit->default_jitter, add_noise ? sigma2 : 0.0, vo.p, st0);
  mo.finish(st0); vo.finish(st0);
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

// d/d xs (gout, d x ns, device) of sum_s mbar_l[s] mean_l(xs_s) + vbar_l[s] var_l(xs_s) summed over the posterior's ms latents
// (DESIGN.md 4.11).  mbar, vbar: ns x ms (column = latent of the shard); vbar == nullptr: the mean-only form (no cross Gram, no solve).
// The full form reuses latent_marginals_dev's batching: cross Gram, R = K(x*, x) L^-T (trsm_rec), W = R L^-1 (trsm_right_rec) on the
// same R buffers, then the pair pass per latent into its slot's accumulator; the slot accumulators are added in slot order after the
// join, so the result does not depend on stream timing.  Caller holds g_mu.
static int mean_var_grad_xs_dev(const lmm_post* P, int ms, const double* xsd, int d, int ns, const double* mbar, const double* vbar,
                                double* gout) {
  hipStream_t st0 = g.streams[0];
  const size_t count = (size_t)d * ns;
  if (vbar == nullptr) {
    Buf<double> part(pred_grad_x_partial_elems(P->n, ns, d));
    for (int k = 0; k < ms; ++k) {
      const Latent& gp = P->ls->lat[P->l0 + k];
      for (int c = 0; c < gp.nt(); ++c)                 // one accumulating pass per term
        launch_pred_grad_x(xsd, ns, P->x.p, P->n, d, P->alpha[k].p, mbar + (size_t)k * ns, nullptr, nullptr, 0,
                           gp.terms[c].ev, part.p, gout, k > 0 || c > 0, st0);
    }
    HIPCHK(hipStreamSynchronize(st0));
    return LMM_OK;
  }
  CrossSlots C(rup(ns, 64));
  FanOut F(ms, mat_bytes(C.elems(P)));
  C.alloc(P, F);
  std::vector<Buf<double>> part, acc;
  for (int s = 0; s < F.nslots; ++s) {
    part.emplace_back(pred_grad_x_partial_elems(P->n, ns, d));
    acc.emplace_back(count);
  }
  std::vector<char> used(F.nslots, 0);
  F.run([&](const FanBatch& b) {
    C.solve(P, b, xsd, d, ns, true, false);                                              // R_j <- K(x*, x) L_j^-T, no split-K
    trsm_right_rec(C.Rb, C.ldr, C.nsr, C.Lb, P->ld, C.Wb, b.nb, 0, P->NC, b.st);         // R_j <- R_j L_j^-1 = K(x*, x) K_j^-1
    for (int j = 0; j < b.nb; ++j) {
      const int k = b.k0 + j;
      const Latent& gp = P->ls->lat[P->l0 + k];
      for (int c = 0; c < gp.nt(); ++c) {
        launch_pred_grad_x(xsd, ns, P->x.p, P->n, d, P->alpha[k].p, mbar + (size_t)k * ns, vbar + (size_t)k * ns, C.R[b.s][j].p, C.ldr,
                           gp.terms[c].ev, part[b.s].p, acc[b.s].p, used[b.s] != 0, b.st);
        used[b.s] = 1;
      }
    }
  });
  sum_slots(gout, acc, used, count, st0, true);
  HIPCHK(hipStreamSynchronize(st0));   // R buffers are released on return
  return LMM_OK;
}

int lmm_oilmm_mean_and_var_grad_xs(const lmm_post_t* post, const lmm_gp_t* gps, const double* U, const double* S, int p, int m,
                                   int latent_begin, int latent_end, const double* xs, int d, int ns,
                                   const double* dmean, const double* dvar, double* grad_xs) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (g_f32) return fail(LMM_ERR_UNSUPPORTED, "gradients of the predictive marginals are served in the Float64 compute mode only");
  if (!U || !xs || !grad_xs || d <= 0 || ns <= 0 || p <= 0 || m <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  if (post && post->kind != 0)
    return fail(LMM_ERR_UNSUPPORTED, "gradients of the predictive marginals of a dense-H posterior (coupled latents) are not served");
  if (int rc = input_grad_check(d, true)) return rc;
  Shard Q;
  if (int rc = post_shard(post, nullptr, gps, m, d, latent_begin, latent_end, Q, "xs")) return rc;
  if (int rc = refuse_sho(*Q.ls, "gradients of the predictive marginals are")) return rc;
  if (int rc = shard_check(Q.l0, Q.l1, m)) return rc;
  const int l0 = Q.l0, ms = Q.ms;
  hipStream_t st0 = g.streams[0];
  const size_t count = (size_t)d * ns;
  DevOut go(grad_xs, count);
  // prior latents: constant means and variances kappa(0); no cotangent, no latent, no work
  if (!post || ms == 0 || (!dmean && !dvar)) {
    HIPCHK(hipMemsetAsync(go.p, 0, count * sizeof(double), st0));
    go.finish(st0);
    HIPCHK(hipStreamSynchronize(st0));
    return LMM_OK;
  }
  // latent cotangents on the device: mbar = dmean H_s, vbar = dvar (H_s .* H_s)   (ns x ms; H_s the shard's columns of U sqrt(S))
  const std::vector<double> Hs = shard_H(U, S, p, l0, ms);
  std::vector<double> HT((size_t)ms * p), H2T((size_t)ms * p);
  for (int k = 0; k < ms; ++k)
    for (int o = 0; o < p; ++o) {
      const double h = Hs[o + (size_t)k * p];
      HT[k + (size_t)o * ms] = h; H2T[k + (size_t)o * ms] = h * h;
    }
  Uploaded HTd(HT, st0), H2Td(H2T, st0);
  DevIn xsd(xs, count, st0), dmd(dmean, (size_t)ns * p, st0), dvd(dvar, (size_t)ns * p, st0);
  Buf<double> mbar((size_t)ns * ms), vbar(dvar ? (size_t)ns * ms : 1);
  if (dmean) launch_tall_skinny(dmd.p, ns, ns, p, HTd.buf.p, ms, ms, mbar.p, ns, nullptr, nullptr, 0, nullptr, 0, st0);
  else HIPCHK(hipMemsetAsync(mbar.p, 0, (size_t)ns * ms * sizeof(double), st0));
  if (dvar) launch_tall_skinny(dvd.p, ns, ns, p, H2Td.buf.p, ms, ms, vbar.p, ns, nullptr, nullptr, 0, nullptr, 0, st0);
  if (int rc = mean_var_grad_xs_dev(post, ms, xsd.p, d, ns, mbar.p, dvar ? vbar.p : nullptr, go.p)) return rc;
  go.finish(st0);
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

// R (nsr x NC, ldr) = K(xs, x) L^-T for latent k of the posterior: the riders of the cross-Gram solved against the factor.
static void cross_solve(const lmm_post* P, int k, const Latent& gp, const double* xsd, int d, int ns, double* Rk, int ldr,
                        int nsr, hipStream_t st) {
  cross_gram(P, gp, xsd, d, ns, Rk, ldr, nsr, st);
  trsm_rec(Rk, ldr, nsr, P->L[k].p, P->ld, P->W[k].p, 0, P->NC, st);
}

// Per-latent posterior (or prior) covariance at xs as a factor matrix B (NRs x NCs): gram(xs) + diag_add - R R' (posterior,
// R from cross_solve), rider row = rider_vec.  Not factorised here (the caller batches potrf_batch).  Caller holds g_mu.
static GramArgs cov_args(const Latent& gp, const double* xsd, int d, int ns, double diag_add, const double* rider_vec,
                         const Dims& Ds, double* B) {
  GramArgs a{};
  a.A = B; a.ld = Ds.ld; a.nrows = Ds.NR; a.ncols = Ds.NC; a.x = xsd; a.d = d; a.n = ns;
  gp.set_kernel(a); a.diag_add = diag_add; a.pad_diag = 1.0;
  a.rider = rider_vec; a.rider_ld = ns; a.nrider = rider_vec ? 1 : 0;
  return a;
}
static void cov_at_xs(const lmm_post* P, const Latent& gp, const double* xsd, int d, int ns, double diag_add,
                      const double* rider_vec, const Dims& Ds, double* B, const double* Rk, int ldr, hipStream_t st) {
  gram_g(cov_args(gp, xsd, d, ns, diag_add, rider_vec, Ds, B), st);
  // Schur complement on the leading NCs x NCs block (rows of R beyond ns are zero)
  if (P != nullptr) gemm_nt_g(B, Ds.ld, Rk, ldr, Rk, ldr, Ds.NC, Ds.NC, P->NC, 1, false, st, "Schur complement (posterior covariance at xs)");
}
// The same for the nb latents of a batch: one Gram launch per run of equal kinds, ONE batched Schur-complement GEMM.
static void cov_at_xs_batch(const lmm_post* P, const GramArgs* ga, int nb, const Dims& Ds, const BatchPtr& Bb, const BatchPtr& Rb,
                            int ldr, hipStream_t st) {
  gram_batch_g(ga, nb, st);
  if (P != nullptr) gemm_nt_g(Bb, 0, Ds.ld, Rb, 0, ldr, Rb, 0, ldr, Ds.NC, Ds.NC, P->NC, 1, false, nb, st, "batched Schur complement (posterior covariance at xs)");
}

// Working buffers of the batched "covariance at xs" loops (rand, posterior logpdf): per stream slot nb_per factor matrices
// with their inverse blocks, means, riders and cross-solve blocks R, and one reduction scratch (reused latent after latent in
// stream order).
struct XsSlots {
  CrossSlots C;                        // the Schur complement reads Ds.NC rows of R (rows beyond ns are zero)
  FanOut F;
  std::vector<std::vector<Buf<double>>> B, WB, mu, rid;
  std::vector<Buf<double>> part;
  XsSlots(const lmm_post* P, int ms, int ns, const Dims& Ds)
      : C(Ds.NC), F(ms, mat_bytes((double)Ds.elems() + (P ? C.elems(P) : 0.0))) {
    const int nslots = F.nslots;
    B.resize(nslots); WB.resize(nslots); mu.resize(nslots); rid.resize(nslots);
    for (int s = 0; s < nslots; ++s) {
      for (int j = 0; j < F.nb_per; ++j) {
        B[s].emplace_back(mat_count(Ds.elems())); WB[s].emplace_back(mat_count((size_t)(Ds.NC / 64) * 4096));
        mu[s].emplace_back((size_t)ns); rid[s].emplace_back((size_t)ns);
      }
      part.emplace_back(std::max(strip_partial_elems(C.nsr, P ? P->NC : 1, 1), strip_partial_elems(ns, ns, 1)));
    }
    if (P) C.alloc(P, F);
  }
  // R[s][j] <- K(xs, x) L_k^-T and mu[s][j] <- mean_k(xs) for the latents of the batch (one batched solve)
  void cross_solve_batch(const lmm_post* P, const FanBatch& b, const double* xsd, int d, int ns) {
    C.solve(P, b, xsd, d, ns, false, false);
    for (int j = 0; j < b.nb; ++j)
      rider_stats_g(C.R[b.s][j].p, C.ldr, ns, P->n, P->z[b.k0 + j].p, P->ls->lat[P->l0 + b.k0 + j].mean, 0.0, part[b.s].p, mu[b.s][j].p,
                    nullptr, b.st);
  }
  // the batch's covariance at xs: one Gram launch per run of equal kinds, ONE batched Schur-complement GEMM against the batch's R
  void cov_batch(const lmm_post* P, const FanBatch& b, const GramArgs* ga, const Dims& Ds) {
    BatchPtr Bb{};
    for (int j = 0; j < b.nb; ++j) Bb.p[j] = B[b.s][j].p;
    cov_at_xs_batch(P, ga, b.nb, Ds, Bb, C.Rb, C.ldr, b.st);
  }
};

extern "C" int lmm_lmm_mean_and_cov(const lmm_post_t* post, const lmm_gp_t* gps, const double* U, const double* S, int p, int m,
                                    int latent_begin, int latent_end, double sigma2, int add_noise, const double* xs, int d,
                                    int ns, const lmm_jitters_t* jit, double* mean_out, double* cov_out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (int rc = post_dtype_check(post)) return rc;
  if (!U || !xs || !mean_out || !cov_out || d <= 0 || ns <= 0 || p <= 0 || m <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  if ((double)p * ns * (double)p * ns > 4e8) return fail(LMM_ERR_UNSUPPORTED, "full covariance (p*ns)^2 too large");
  if (!jit) jit = &kDefaultJit;
  const lmm_post* P = post;
  Shard Q;
  if (int rc = post_shard(P, "full covariance of the dense-H posterior is not built", gps, m, d, latent_begin, latent_end, Q)) return rc;
  if (int rc = shard_check(Q.l0, Q.l1, m)) return rc;
  const Latent* lts = Q.lts;
  const int l0 = Q.l0, ms = Q.ms;
  hipStream_t st0 = g.streams[0];
  const std::vector<double> Hs = shard_H(U, S, p, l0, ms);
  Uploaded Hd(Hs, st0);
  DevIn xsd(xs, (size_t)d * ns, st0);
  DevOut mo(mean_out, (size_t)ns * p), co(cov_out, (size_t)ns * p * ns * p);
  Buf<double> ml((size_t)ns * std::max(ms, 1));
  Dims Ds(ns, 0);
  const int nsr = Ds.NC;           // the Schur complement reads Ds.NC rows of R
  const int ldr = pad_ld(nsr);
  const int CH = LMM_MAX_BATCH;
  std::vector<Buf<double>> Cm;
  for (int c = 0; c < std::min(CH, std::max(ms, 1)); ++c) Cm.emplace_back(mat_count(Ds.elems()));
  Buf<double> R(P ? mat_count((size_t)ldr * P->NC) : 1), part(strip_partial_elems(nsr, P ? P->NC : 1, 1));
  if (ms == 0) {
    HIPCHK(hipMemsetAsync(mo.p, 0, (size_t)ns * p * sizeof(double), st0));
    BatchPtr none{};
    launch_cov_mix(none, Ds.ld, 0, Hd.buf.p, p, ns, 0.0, add_noise ? sigma2 : 0.0, 1, co.p, st0);
  }
  for (int k0 = 0; k0 < ms; k0 += CH) {
    const int nl = std::min(CH, ms - k0);
    BatchPtr cl{};
    for (int j = 0; j < nl; ++j) {
      const int k = k0 + j;
      const Latent& gp = lts[l0 + k];
      if (P) cross_solve(P, k, gp, xsd.p, d, ns, R.p, ldr, nsr, st0);
      rider_stats_g(P ? R.p : nullptr, ldr, ns, P ? P->n : 0, P ? P->z[k].p : nullptr, gp.mean, 0.0, part.p,
                         ml.p + (size_t)k * ns, nullptr, st0);
      cov_at_xs(P, gp, xsd.p, d, ns, 0.0, nullptr, Ds, Cm[j].p, R.p, ldr, st0);
      cl.p[j] = Cm[j].p;
    }
    launch_cov_mix(cl, Ds.ld, nl, Hd.buf.p + (size_t)k0 * p, p, ns, jit->default_jitter, add_noise ? sigma2 : 0.0,
                   k0 == 0 ? 1 : 0, co.p, st0);
  }
  if (ms > 0) launch_mix(ml.p, ns, ms, Hd.buf.p, p, 1, 0.0, 0.0, nullptr, 0.0, mo.p, st0);
  mo.finish(st0); co.finish(st0);
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

// cov(f::IndependentMOGP, x, y): reference src/independent_mogp.jl:66-71 (both inputs by outputs) and :184-215 (by features / mixed:
// the same blocks at permuted rows / columns).  Block l = cov(f_l, x.x, y.x): kernelmatrix(k_l, x, y) for a prior latent,
// K(x, y) - A_x' A_y with A_z = C.U' \ K(x_train, z) for a PosteriorGP latent (AbstractGPs).
extern "C" int lmm_mogp_cross_cov(const lmm_post_t* post, const lmm_gp_t* gps, int m, int latent_begin, int latent_end,
                                  const double* x, int d, int n, int x_by_features, const double* y, int n2, int y_by_features,
                                  double* cov_out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (int rc = post_dtype_check(post)) return rc;
  if (!x || !y || !cov_out || d <= 0 || n <= 0 || n2 <= 0 || m <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  if ((double)m * n * (double)m * n2 > 4e8) return fail(LMM_ERR_UNSUPPORTED, "cross-covariance (m n) x (m n2) too large");
  const lmm_post* P = post;
  Shard Q;
  if (int rc = post_shard(P, "cross-covariance of the coupled latents of a dense-H posterior is not built", gps, m, d, latent_begin, latent_end, Q, "x",
                          "posterior has %d latents, m = %d")) return rc;
  if (int rc = shard_check(Q.l0, Q.l1, m)) return rc;
  const Latent* lts = Q.lts;
  const int l0 = Q.l0, l1 = Q.l1;
  hipStream_t st0 = g.streams[0];
  DevIn xd(x, (size_t)d * n, st0), yd(y, (size_t)d * n2, st0);
  const size_t R = (size_t)m * n, Ccols = (size_t)m * n2;
  DevOut co(cov_out, R * Ccols);
  HIPCHK(hipMemsetAsync(co.p, 0, R * Ccols * sizeof(double), st0));        // the off-diagonal blocks (and latents outside the shard)
  // K(x, y) as the "rider rows" of a Gram launch whose column points are y: rows [NCy, NCy + nxr) of a (NCy + nxr) x NCy layout,
  // stored from buffer row 0 (the cross-Gram form of the predictive paths)
  const int nxr = rup(n, 128), NCy = rup(n2, 128);
  const int ldk = pad_ld(nxr);
  Buf<double> Kb(mat_count((size_t)ldk * NCy));
  const int ldr = pad_ld(std::max(nxr, NCy));
  Buf<double> Rx(P ? mat_count((size_t)ldr * P->NC) : 1), Ry(P ? mat_count((size_t)ldr * P->NC) : 1);
  for (int l = l0; l < l1; ++l) {
    const Latent& gp = lts[l];
    GramArgs a{};
    a.A = Kb.p; a.ld = ldk; a.nrows = NCy + nxr; a.ncols = NCy; a.row_tile0 = NCy / 64; a.row_shift = NCy; a.full = 1;
    a.x = yd.p; a.d = d; a.n = n2; gp.set_kernel(a);
    a.xs = xd.p; a.ns = n;
    gram_g(a, st0, "cross-covariance K(x, y)");
    if (P) {
      const int k = l - l0;
      cross_solve(P, k, gp, xd.p, d, n, Rx.p, ldr, nxr, st0);              // R_x = K(x, X) L^-T
      cross_solve(P, k, gp, yd.p, d, n2, Ry.p, ldr, NCy, st0);             // R_y = K(y, X) L^-T
      gemm_nt_g(Kb.p, ldk, Rx.p, ldr, Ry.p, ldr, nxr, NCy, P->NC, 0, false, st0, "cross-covariance Schur complement");
    }
    launch_block_scatter(Kb.p, ldk, n, n2, co.p, R, x_by_features ? (size_t)l : (size_t)l * n, x_by_features ? m : 1,
                         y_by_features ? (size_t)l : (size_t)l * n2, y_by_features ? m : 1, st0);
  }
  co.finish(st0);
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

int lmm_oilmm_post_logpdf(const lmm_post_t* post, const double* U, const double* S, int p, int m, double sigma2,
                          const double* xs, int d, int ns, const double* ys, int with_regulariser, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (int rc = post_dtype_check(post)) return rc;
  if (!post || !U || !S || !xs || !ys || !out || d <= 0 || ns <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  const lmm_post* P = post;
  Shard Q;
  if (int rc = post_shard(P, "dense-H posterior handle: use lmm_ilmm_post_logpdf", nullptr, m, d, 0, 0, Q)) return rc;
  if (m > p) return fail(LMM_ERR_DIM, "out dim of x != out dim of f.");
  if (!(sigma2 > 0.0)) return fail(LMM_ERR_ARG, "sigma2 must be > 0");
  hipStream_t st0 = g.streams[0];
  const int l0 = Q.l0, ms = Q.ms;
  OilmmFront F(U, S, p, m, sigma2);
  const std::vector<double>& ST = F.ST;
  DevIn xsd(xs, (size_t)d * ns, st0), ysd(ys, (size_t)ns * p, st0);
  F.Td = Uploaded(F.T, st0);      // (the handle's vectors carry the means)
  double resid = 0.0;
  const double* Ty_shard = F.rows(ysd.p, ns, l0, ms, with_regulariser != 0, &resid);
  if (with_regulariser) HIPCHK(hipStreamSynchronize(st0));
  Dims Ds(ns, 1);
  XsSlots X(P, ms, ns, Ds);
  const int mk = X.F.mk;
  Buf<double> outd(mk);
  int* info = X.F.alloc_info();
  X.F.run([&](const FanBatch& b) {
    const int s = b.s, nb = b.nb;
    hipStream_t st = b.st;
    Batch Bt;
    X.cross_solve_batch(P, b, xsd.p, d, ns);
    GramArgs ga[LMM_MAX_BATCH];
    for (int j = 0; j < nb; ++j) {
      const int k = b.k0 + j;
      const Latent& gp = P->ls->lat[l0 + k];
      launch_vec_lin(Ty_shard + (size_t)k * ns, X.mu[s][j].p, -1.0, ns, X.rid[s][j].p, st);
      ga[j] = cov_args(gp, xsd.p, d, ns, ST[l0 + k], X.rid[s][j].p, Ds, X.B[s][j].p);
      Bt.add(X.B[s][j].p, X.WB[s][j].p, info + k);
    }
    X.cov_batch(P, b, ga, Ds);
    potrf_batch(Bt, Ds.ld, Ds.NR, Ds.NC, ns, st);
    launch_lml_reduce(Bt.A, nb, Ds.ld, ns, Ds.NC, 1, outd.p + b.k0, st);
  });
  std::vector<double> lml(mk, 0.0);
  HIPCHK(hipMemcpyAsync(lml.data(), outd.p, mk * sizeof(double), hipMemcpyDeviceToHost, st0));
  if (int rc = X.F.check(l0)) return rc;
  double total = 0.0;
  for (int k = 0; k < ms; ++k) total += lml[k];
  if (with_regulariser) total += oilmm_regulariser(ns, p, m, S, sigma2, resid);
  *out = total;
  return LMM_OK;
  LMM_CATCH
}

int lmm_lmm_rand_multi(const lmm_post_t* post, const lmm_gp_t* gps, const double* U, const double* S, int p, int m,
                       int latent_begin, int latent_end, double sigma2, int add_noise, const double* xs, int d, int ns,
                       int nsamples, const double* z_lat, const double* eps, const lmm_jitters_t* jit, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (int rc = post_dtype_check(post)) return rc;
  if (!U || !xs || !z_lat || !out || d <= 0 || ns <= 0 || p <= 0 || m <= 0 || nsamples <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  if (add_noise && !eps) return fail(LMM_ERR_ARG, "eps is NULL");
  if (!jit) jit = &kDefaultJit;
  const lmm_post* P = post;
  Shard Q;
  if (int rc = post_shard(P, "dense-H posterior handle: use lmm_ilmm_post_rand", gps, m, d, latent_begin, latent_end, Q)) return rc;
  if (int rc = shard_check(Q.l0, Q.l1, m)) return rc;
  const Latent* lts = Q.lts;
  const int l0 = Q.l0, ms = Q.ms, mk = Q.mk;
  // OILMM: f(x) default jitter 1e-18 (reference src/oilmm.jl:47); dense-H ILMM: 1e-12 (src/ilmm.jl:84)
  const double jitter = S ? jit->default_jitter : jit->ilmm_rand_jitter;
  hipStream_t st0 = g.streams[0];
  const std::vector<double> Hs = shard_H(U, S, p, l0, ms);
  Uploaded Hd(Hs, st0);
  // z_lat: [sample][m][ns], eps: [sample][p][ns], out: [sample][p][ns]
  DevIn xsd(xs, (size_t)d * ns, st0), zd(z_lat, (size_t)ns * m * nsamples, st0);
  DevIn epsd(add_noise ? eps : nullptr, (size_t)ns * p * nsamples, st0);
  Dims Ds(ns, 0);
  XsSlots Xs(P, ms, ns, Ds);
  Buf<double> X((size_t)ns * mk * nsamples);     // [sample][latent of the shard][ns]
  int* info = Xs.F.alloc_info();
  Xs.F.run([&](const FanBatch& b) {
    const int s = b.s, nb = b.nb;
    hipStream_t st = b.st;
    Batch Bt;
    if (P) Xs.cross_solve_batch(P, b, xsd.p, d, ns);      // posterior: R_k and the mean vectors (sample = mean + L z)
    GramArgs ga[LMM_MAX_BATCH];
    for (int j = 0; j < nb; ++j) {
      const int k = b.k0 + j;
      ga[j] = cov_args(lts[l0 + k], xsd.p, d, ns, jitter, nullptr, Ds, Xs.B[s][j].p);
      Bt.add(Xs.B[s][j].p, Xs.WB[s][j].p, info + k);
    }
    Xs.cov_batch(P, b, ga, Ds);
    potrf_batch(Bt, Ds.ld, Ds.NR, Ds.NC, ns, st);      // ONE factorisation per latent, nsamples triangular products
    for (int j = 0; j < nb; ++j) {
      const int k = b.k0 + j;
      const double mu_const = P ? 0.0 : lts[l0 + k].mean;
      for (int q = 0; q < nsamples; ++q) {
        double* Xq = X.p + ((size_t)q * ms + k) * ns;
        launch_trmv_lower(Xs.B[s][j].p, Ds.ld, ns, zd.p + ((size_t)q * m + l0 + k) * ns, mu_const, Xs.part[s].p, Xq, st);
        if (P) launch_vec_lin(Xq, Xs.mu[s][j].p, 1.0, ns, Xq, st);
      }
    }
  });
  DevOut od(out, (size_t)ns * p * nsamples);
  // reference src/oilmm.jl:50-53 / src/ilmm.jl:86: F = vec((H X')') + sqrt(sigma2) eps
  for (int q = 0; q < nsamples; ++q)
    launch_mix(X.p + (size_t)q * ms * ns, ns, ms, Hd.buf.p, p, 1, 0.0, 0.0, add_noise ? epsd.p + (size_t)q * ns * p : nullptr,
               std::sqrt(sigma2), od.p + (size_t)q * ns * p, st0);
  od.finish(st0);
  return Xs.F.check(l0);
  LMM_CATCH
}

int lmm_lmm_rand(const lmm_post_t* post, const lmm_gp_t* gps, const double* U, const double* S, int p, int m,
                 int latent_begin, int latent_end, double sigma2, int add_noise, const double* xs, int d, int ns,
                 const double* z_lat, const double* eps, const lmm_jitters_t* jit, double* out) {
  return lmm_lmm_rand_multi(post, gps, U, S, p, m, latent_begin, latent_end, sigma2, add_noise, xs, d, ns, 1, z_lat, eps, jit, out);
}

// ------------------------------------------------------------------------------------------------
// inducing points (VFE)
// ------------------------------------------------------------------------------------------------
#define LMM_SPARSE_POST_MAGIC 0x56464531     // a handle of another kind handed to a sparse entry point is refused, not read
struct lmm_sparse_post {
  int magic = LMM_SPARSE_POST_MAGIC;
  int d = 0, nz = 0, l0 = 0, l1 = 0, m = 0;
  int NC = 0, NR = 0, ld = 0;
  std::shared_ptr<LatentSet> ls;
  Buf<double> z;                            // d x nz
  std::vector<Buf<double>> Lu, Wu;          // per latent of the shard: factor of K_uu + jitter I and its inverse diagonal blocks
  std::vector<Buf<double>> LB, WB;          // the same for B = I + L_u^-1 Phi L_u^-T
  std::vector<Buf<double>> c;               // L_B^-1 L_u^-1 b (NC values, zero beyond nz)
};

// What the n data points contribute, and the two M x M factorisations, for the latents [l0, l1).
struct SparseState {
  std::vector<Buf<double>> Lu, Wu, LB, WB, c;
  std::vector<double> dtc, elbo;            // per latent of the shard
  bool keep_grad = false;                   // the gradient's inputs: Q = L_u^-1 Phi L_u^-T per latent and the scalars s, kappa, c'c
  std::vector<Buf<double>> Q;
  std::vector<double> s, kappa, ctc;
};

static int sparse_size_check(int d, int nz) {      // what the kernels are built for; all the one-latent building blocks check
  if (nz > LMM_SPARSE_MMAX) return fail(LMM_ERR_UNSUPPORTED, "inducing-point inference is served for at most %d inducing points (nz = %d)", LMM_SPARSE_MMAX, nz);
  if (d > LMM_SPARSE_DMAX) return fail(LMM_ERR_UNSUPPORTED, "inducing-point inference is served for d <= %d (d = %d)", LMM_SPARSE_DMAX, d);
  return LMM_OK;
}
static int sparse_shape_check(int d, int nz, double jitter) {
  if (int rc = sparse_size_check(d, nz)) return rc;
  if (g_f32) return fail(LMM_ERR_UNSUPPORTED, "inducing-point inference is Float64 only (lmm_set_compute_dtype(LMM_F64))");
  if (!(jitter > 0.0) || !std::isfinite(jitter)) return fail(LMM_ERR_ARG, "jitter must be finite and > 0");
  return LMM_OK;
}

static void sparse_fill_lat(SparseLat& s, const Latent& gp, const double* w, double wconst, const double* r, double rsub) {
  s.g = gp.dev(); s.w = w; s.wconst = wconst; s.r = r; s.rsub = rsub; s.kdiag = gp.prior_var();
  s.sum_per = gp.is_sum() && gp.has_periodic();
}

// Partials per chunk for nb latents: checks an explicit chunk, or picks the default.
static int sparse_plan(int n, int nz, int nb, int chunk, int* chunk_out, int* nch_out) {
  if (chunk < 0) return fail(LMM_ERR_ARG, "chunk must be >= 0");
  if (chunk == 0) chunk = sparse_default_chunk(n, nz, nb);
  const long long nch = ((long long)n + chunk - 1) / chunk;
  if (nch > 65535 || (double)nch * nb * (double)sparse_partial_stride(nz) * 8.0 > 2e9)
    return fail(LMM_ERR_ARG, "chunk = %d gives %lld partials for n = %d: too many (raise chunk, or pass 0)", chunk, nch, n);
  *chunk_out = chunk; *nch_out = (int)nch;
  return LMM_OK;
}
struct SparsePoints { const double* x; int d, n; const double* z; int nz, chunk, nch; };      // what a pass over the points walks (sparse_plan)

// The first pass over the points for nb latents (a.lat[0 .. nb), sparse_fill_lat): the moments per chunk, then their sums into Phi
// (ld; zero_pad: its pad rows and columns too), b and the scalars.
static void sparse_moments_pass(SparseMomArgs& a, const SparsePoints& P, double* scratch, int nb, int mode, const BatchPtr& Phi, int ld,
                                bool zero_pad, const BatchPtr& b, const BatchPtr& scalars, hipStream_t st) {
  a.x = P.x; a.z = P.z; a.d = P.d; a.n = P.n; a.nz = P.nz; a.chunk = P.chunk; a.nch = P.nch; a.scratch = scratch;
  launch_sparse_moments(a, nb, mode, st);
  launch_sparse_finish(scratch, P.nch, P.nz, Phi, ld, zero_pad, b, scalars, nb, st);
}
// The second pass for nb latents (hlat[0 .. nb), sparse_grad_fill_lat; dlat: their device copy, the caller's): the K_uf sums per chunk,
// then the term records and d/dz (gz entries may be nullptr).
static void sparse_grad_pass(const SparseGradLat* hlat, SparseGradLat* dlat, const SparsePoints& P, int ld, double* scratch, int nb, int mode,
                             const BatchPtr& records, const BatchPtr& gz, hipStream_t st) {
  HIPCHK(hipMemcpyAsync(dlat, hlat, (size_t)nb * sizeof(SparseGradLat), hipMemcpyHostToDevice, st));
  SparseGradArgs a{};
  a.x = P.x; a.z = P.z; a.d = P.d; a.n = P.n; a.nz = P.nz; a.chunk = P.chunk; a.nch = P.nch; a.ld = ld; a.scratch = scratch; a.lat = dlat;
  launch_sparse_grad(a, nb, mode, st);
  launch_sparse_grad_finish(scratch, P.nch, P.nz, P.d, records, gz, nb, st);
}

// rv: device, the projected data of latent l0 + k at rv + k * n (its mean rsub[l0 + k] is subtracted by the kernel); wconst[l0 + k]: its
// noise.  keep: the factors stay in `out` (posterior), else only dtc / elbo are filled.  Caller holds g_mu; runs on streams[0].
static int sparse_core(const double* xd, int d, int n, const double* zd, int nz, double jitter, const Latent* lts, int l0, int l1,
                       const double* rv, const double* rsub, const double* wconst, SparseState& out) {
  const int ms = l1 - l0, M = nz;
  out.dtc.assign(ms, 0.0); out.elbo.assign(ms, 0.0);
  if (ms == 0) return LMM_OK;
  hipStream_t st = g.streams[0];
  Dims D(M, 1);
  FanOut F = FanOut::one_slot(ms);
  const int nb_per = F.nb_per;
  for (int k = 0; k < ms; ++k) {
    out.Lu.emplace_back(D.elems()); out.Wu.emplace_back((size_t)(D.NC / 64) * 4096);
    out.LB.emplace_back(D.elems()); out.WB.emplace_back((size_t)(D.NC / 64) * 4096);
    out.c.emplace_back((size_t)D.NC);
  }
  std::vector<Buf<double>> Q;                // one per batch slot, or (keep_grad) one per latent
  for (int j = 0; j < (out.keep_grad ? ms : nb_per); ++j) Q.emplace_back(D.elems());
  // b (NC per latent); res = [3 ms: s, kappa, lambda | ms: tr Q | 2 ms: -(M log 2pi + log det B + q) / 2 with q = c'c, then q = 0 (the zero row under the rider)]; two pivot-info words per latent
  Buf<double> bvec((size_t)D.NC * ms), res((size_t)6 * ms);
  int* info = F.alloc_info(2);
  int chunk = 0, nch = 0;
  if (int rc = sparse_plan(n, nz, nb_per, 0, &chunk, &nch)) return rc;
  Buf<double> scratch((size_t)nb_per * nch * sparse_partial_stride(nz));
  F.run([&](const FanBatch& fb) {
    const int k0 = fb.k0, nb = fb.nb;
    SparseMomArgs a{};
    BatchPtr Pb{}, Qb{}, bb{}, sb{};
    Batch Bu, Bb;
    GramArgs ga[LMM_MAX_BATCH];
    for (int j = 0; j < nb; ++j) {
      const int k = k0 + j;
      const Latent& gp = lts[l0 + k];
      sparse_fill_lat(a.lat[j], gp, nullptr, wconst[l0 + k], rv + (size_t)k * n, rsub[l0 + k]);
      Pb.p[j] = out.LB[k].p; Qb.p[j] = Q[out.keep_grad ? k : j].p; bb.p[j] = bvec.p + (size_t)k * D.NC; sb.p[j] = res.p + (size_t)3 * k;
      HIPCHK(hipMemsetAsync(out.LB[k].p, 0, D.elems() * sizeof(double), st));      // Phi's pad rows and columns
      GramArgs r{};
      r.A = out.Lu[k].p; r.ld = D.ld; r.nrows = D.NR; r.ncols = D.NC; r.x = zd; r.d = d; r.n = M;
      gp.set_kernel(r); r.pad_diag = 1.0; r.diag_add = jitter;
      r.rider = bb.p[j]; r.rider_ld = D.NC; r.nrider = 1;
      ga[j] = r;
      Bu.add(out.Lu[k].p, out.Wu[k].p, info + k);
      Bb.add(out.LB[k].p, out.WB[k].p, info + ms + k);
    }
    sparse_moments_pass(a, SparsePoints{xd, d, n, zd, nz, chunk, nch}, scratch.p, nb, sum_mode(lts, l0 + k0, l0 + k0 + nb), Pb, D.ld, true, bb, sb, st);
    // L_u = chol(K_uu + jitter I), with b as the rider row: it becomes c0 = L_u^-1 b
    gram_batch_g(ga, nb, st, "inducing Gram assembly");
    potrf_batch(Bu, D.ld, D.NR, D.NC, M, st, D.NC + 1);
    // Q = L_u^-1 Phi L_u^-T: Phi L_u^-T, transposed, solved again (Phi is symmetric)
    trsm_rec(Pb, D.ld, D.NC, Bu.A, D.ld, Bu.W, nb, 0, D.NC, st, false, true, true);      // (no split-K atomics: M x M work)
    launch_sparse_transpose(Pb, Qb, D.ld, D.NC, nb, st);
    trsm_rec(Qb, D.ld, D.NC, Bu.A, D.ld, Bu.W, nb, 0, D.NC, st, false, true, true);
    // B = I + Q with the rider c0 (overwrites the Phi buffer), L_B = chol(B), rider c = L_B^-1 c0
    for (int j = 0; j < nb; ++j) guard_extent(Pb.p[j], D.NR, D.ld, D.NC, true, "B assembly");
    launch_sparse_bmat(Qb, Bu.A, Pb, D.ld, D.NC, D.NR, M, res.p + (size_t)3 * ms + k0, nb, st);
    potrf_batch(Bb, D.ld, D.NR, D.NC, M, st, D.NC + 1);
    launch_lml_reduce(Bb.A, nb, D.ld, M, D.NC, 2, res.p + (size_t)4 * ms + (size_t)2 * k0, st);
    BatchPtr cb{};
    for (int j = 0; j < nb; ++j) cb.p[j] = out.c[k0 + j].p;
    launch_extract_rows(Bb.A, nb, D.ld, D.NC, M, D.NC, cb, cb, st);
  });
  std::vector<double> hres((size_t)6 * ms);
  HIPCHK(hipMemcpyAsync(hres.data(), res.p, hres.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  const int* hinfo = F.host_info();
  if (int rc = check_info(hinfo, ms, l0)) { if (rc == LMM_ERR_NOT_PD) g.err += " [K_uu + jitter I of the inducing points]"; return rc; }
  if (int rc = check_info(hinfo + ms, ms, l0)) { if (rc == LMM_ERR_NOT_PD) g.err += " [B = I + L_u^-1 Phi L_u^-T]"; return rc; }
  for (int k = 0; k < ms; ++k) {
    const double* r = hres.data() + (size_t)3 * k;       // s, kappa, lambda
    // the Gaussian form carries -c'c / 2, the bound +c'c / 2: c'c = 2 (g0 - gc) from the two reductions
    const double gc = hres[(size_t)4 * ms + 2 * k], g0 = hres[(size_t)4 * ms + 2 * k + 1];
    out.dtc[k] = 2.0 * g0 - gc + 0.5 * M * kLog2Pi - 0.5 * ((double)n * kLog2Pi + r[2] + r[0]);
    out.elbo[k] = out.dtc[k] - 0.5 * (r[1] - hres[(size_t)3 * ms + k]);
    if (out.keep_grad) { out.s.push_back(r[0]); out.kappa.push_back(r[1]); out.ctc.push_back(2.0 * (g0 - gc)); }
  }
  if (out.keep_grad) out.Q = std::move(Q);
  return LMM_OK;
}


// ---- gradient of the bound ----------------------------------------------------------------------------------------
// Per latent l, un-whitened: K = K_uu + jitter I, Sigma = K + Phi, beta = Sigma^-1 b,
//     PhiBar = d elbo_l / d Phi = (K^-1 - Sigma^-1 - beta beta') / 2,   KuuBar = d elbo_l / d K_uu = PhiBar - K^-1 Phi K^-1 / 2,
// from the forward pass's factors: X' = L_u^-T (identity riders through trsm_rec), Y' = X' L_B^-T, K^-1 = X'X, Sigma^-1 = Y'Y,
// beta = Y' c, K^-1 Phi K^-1 = X' Q X.  The second pass over the points (sparse_grad_kernel) contracts g = (2 PhiBar K_uf + beta r') / w with
// d k; the K_uu terms are the gradient reductions of the exact path over x = z with alpha = 0 and -2 KuuBar as the inverse.
static void sparse_grad_fill_lat(SparseGradLat& s, const Latent& gp, const LatentDev* gd, const double* w, double wconst, const double* r,
                                 double rsub, const double* PhiBar, const double* beta, double* grad_r) {
  s.g = gp.dev(); s.gd = gd; s.nterms = gp.nt();
  s.w = w; s.wconst = wconst; s.r = r; s.rsub = rsub; s.PhiBar = PhiBar; s.beta = beta; s.grad_r = grad_r;
}

// hred: LMM_NGRAD sums per term of the latents [l0, l1) (K_uf and K_uu contributions added; [1] of a latent's first term: tr(-2 KuuBar)),
// hard: d per-dimension sums per term; gksum: sum_{i,t} g_it k(z_i, x_t) per latent (the K_uf share of [7] over its terms); gr_dev: d elbo / d r, n per latent; gz_dev: d x nz summed over the latents, or nullptr.
static int sparse_grad_core(const double* xd, int d, int n, const double* zd, int nz, const LatentSet* ls, int l0, int l1, const double* rv,
                            const double* rsub, const double* wconst, const SparseState& S, std::vector<double>& hred,
                            std::vector<double>& hard, std::vector<double>& gksum, double* gr_dev, double* gz_dev) {
  const Latent* lts = ls->lat.data();
  const int ms = l1 - l0, M = nz, NGR = LMM_NGRAD, no = LMM_NGRAD + d;
  hipStream_t st = g.streams[0];
  const std::vector<int> toff = ls->term_offsets(l0, l1);
  const int nterm = toff[ms];
  hred.assign((size_t)NGR * std::max(nterm, 1), 0.0); hard.assign((size_t)d * std::max(nterm, 1), 0.0);
  gksum.assign(std::max(ms, 1), 0.0);
  if (gz_dev) HIPCHK(hipMemsetAsync(gz_dev, 0, (size_t)d * nz * sizeof(double), st));
  if (ms == 0) return LMM_OK;
  Dims D(M, 1);
  FanOut fan = FanOut::one_slot(ms);
  const int nb_per = fan.nb_per;
  std::vector<LatentDev> hgd;
  for (int k = 0; k < ms; ++k) for (const KernelTerm& T : lts[l0 + k].terms) hgd.push_back(T.gd);
  Buf<LatentDev> gdd(nterm);
  HIPCHK(hipMemcpyAsync(gdd.p, hgd.data(), hgd.size() * sizeof(LatentDev), hipMemcpyHostToDevice, st));
  std::vector<SparseGradLat> hlat(nb_per);
  Buf<SparseGradLat> dlat(nb_per);
  std::vector<Buf<double>> Ru, Ki, Si, T1, T2, gzl;      // five M x M buffers per batch slot (Y' is built in place of X')
  for (int j = 0; j < nb_per; ++j) {
    Ru.emplace_back(D.elems()); Ki.emplace_back(D.elems()); Si.emplace_back(D.elems());
    T1.emplace_back(D.elems()); T2.emplace_back(D.elems());
    if (gz_dev) gzl.emplace_back((size_t)d * nz);
  }
  const size_t nrec = (size_t)LMM_SUM_MAX_TERMS * no;
  Buf<double> beta((size_t)D.NC * ms), recF(nrec * ms), recK((size_t)NGR * nterm), ardK((size_t)d * nterm), zeros((size_t)D.NC);
  Buf<double> gpart((size_t)grad_partials(M, d)), gxpart(gz_dev ? grad_x_partial_elems(M, d) : 1);
  HIPCHK(hipMemsetAsync(recK.p, 0, (size_t)NGR * nterm * sizeof(double), st));
  HIPCHK(hipMemsetAsync(ardK.p, 0, (size_t)d * nterm * sizeof(double), st));
  HIPCHK(hipMemsetAsync(zeros.p, 0, (size_t)D.NC * sizeof(double), st));
  int chunk = 0, nch = 0;
  if (int rc = sparse_plan(n, nz, nb_per, 0, &chunk, &nch)) return rc;
  const int tm = (nz + 63) / 64;
  Buf<double> scratch((size_t)nb_per * nch * tm * sparse_grad_partial_stride(d));
  const int mode = sum_mode(lts, l0, l1);
  bool gz_first = true;
  fan.run([&](const FanBatch& fb) {
    const int k0 = fb.k0, nb = fb.nb;
    BatchPtr Rub{}, Kib{}, Sib{}, T1b{}, T2b{}, Lub{}, Wub{}, LBb{}, WBb{}, Qb{}, cb{}, betab{}, recb{}, gzb{};
    for (int j = 0; j < nb; ++j) {
      const int k = k0 + j;
      Rub.p[j] = Ru[j].p; Kib.p[j] = Ki[j].p; Sib.p[j] = Si[j].p; T1b.p[j] = T1[j].p; T2b.p[j] = T2[j].p;
      Lub.p[j] = S.Lu[k].p; Wub.p[j] = S.Wu[k].p; LBb.p[j] = S.LB[k].p; WBb.p[j] = S.WB[k].p; Qb.p[j] = S.Q[k].p; cb.p[j] = S.c[k].p;
      betab.p[j] = beta.p + (size_t)k * D.NC; recb.p[j] = recF.p + nrec * k; gzb.p[j] = gz_dev ? gzl[j].p : nullptr;
      launch_set_identity(Ru[j].p, D.ld, D.NC, st);
      HIPCHK(hipMemsetAsync(T1[j].p, 0, D.elems() * sizeof(double), st));
      HIPCHK(hipMemsetAsync(T2[j].p, 0, D.elems() * sizeof(double), st));
    }
    trsm_rec(Rub, D.ld, D.NC, Lub, D.ld, Wub, nb, 0, D.NC, st, true, true, true);          // X' = L_u^-T (upper triangular)
    launch_syrk_upper_set(Kib, D.ld, Rub, D.ld, D.NC, nb, st);                             // lower(Ki) = X'X = K^-1
    // T2 = X' Q' X = K^-1 Phi K^-1 through two C -= A B' products (no split-K atomics: M x M work)
    gemm_nt_g(T1b, 0, D.ld, Rub, 0, D.ld, Qb, 0, D.ld, D.NC, D.NC, D.NC, 0, false, nb, st, "K^-1 Phi K^-1 (first product)", true);
    gemm_nt_g(T2b, 0, D.ld, T1b, 0, D.ld, Rub, 0, D.ld, D.NC, D.NC, D.NC, 0, false, nb, st, "K^-1 Phi K^-1 (second product)", true);
    trsm_rec(Rub, D.ld, D.NC, LBb, D.ld, WBb, nb, 0, D.NC, st, false, true, true);         // in place: Y' = X' L_B^-T (upper triangular)
    launch_syrk_upper_set(Sib, D.ld, Rub, D.ld, D.NC, nb, st);                             // lower(Si) = Y'Y = Sigma^-1
    launch_sparse_beta(Rub, D.ld, M, cb, betab, nb, st);
    launch_sparse_phibar(Kib, Sib, T2b, betab, T1b, D.ld, M, nb, st);                      // T1 <- PhiBar, lower(Si) <- -2 KuuBar
    for (int j = 0; j < nb; ++j) {
      const int k = k0 + j;
      sparse_grad_fill_lat(hlat[j], lts[l0 + k], gdd.p + toff[k], nullptr, wconst[l0 + k], rv + (size_t)k * n, rsub[l0 + k], T1[j].p,
                           betab.p[j], gr_dev + (size_t)k * n);
    }
    sparse_grad_pass(hlat.data(), dlat.p, SparsePoints{xd, d, n, zd, nz, chunk, nch}, D.ld, scratch.p, nb, mode, recb, gzb, st);
    for (int j = 0; j < nb; ++j) {
      const int k = k0 + j;
      for (int c = 0; c < lts[l0 + k].nt(); ++c) {
        const LatentDev& gd = lts[l0 + k].terms[c].gd;
        const size_t t = (size_t)toff[k] + c;
        launch_grad_reduce(Si[j].p, D.ld, M, M, zeros.p, zeros.p, zd, d, gd, gpart.p, recK.p + NGR * t, st, ardK.p + d * t);
        if (gz_dev) launch_grad_x(Si[j].p, D.ld, M, zeros.p, zd, d, gd, gxpart.p, gzl[j].p, true, st);
      }
      if (gz_dev) {                              // the latents in order
        if (gz_first) HIPCHK(hipMemcpyAsync(gz_dev, gzl[j].p, (size_t)d * nz * sizeof(double), hipMemcpyDeviceToDevice, st));
        else launch_vec_lin(gz_dev, gzl[j].p, 1.0, d * nz, gz_dev, st);
        gz_first = false;
      }
    }
    HIPCHK(hipStreamSynchronize(st));            // hlat is rewritten by the next batch
  });
  std::vector<double> hF(nrec * ms), hK((size_t)NGR * nterm), hA((size_t)d * nterm);
  HIPCHK(hipMemcpyAsync(hF.data(), recF.p, hF.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hK.data(), recK.p, hK.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hA.data(), ardK.p, hA.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  static const int slots[4] = {0, 7, 8, 9};
  for (int k = 0; k < ms; ++k)
    for (int c = 0; c < lts[l0 + k].nt(); ++c) {
      const size_t t = (size_t)toff[k] + c;
      const double* F = &hF[nrec * k + (size_t)no * c];
      for (int e : slots) hred[NGR * t + e] = F[e] + hK[NGR * t + e];
      hred[NGR * t + 1] = hK[NGR * t + 1];
      gksum[k] += F[7];
      const bool ard = lts[l0 + k].terms[c].gd.ils != nullptr;
      for (int kk = 0; kk < d; ++kk) hard[(size_t)d * t + kk] = F[NGR + kk] + (ard ? hA[(size_t)d * t + kk] : 0.0);
    }
  return LMM_OK;
}

// The front end of the inducing-point entry points.  sparse_resolve, in the order the error codes are pinned in: `bad` (the entry
// point's own NULL test, or a NULL / size defect of the shared arguments), m > p and the shard, the shape (nz, d, dtype, jitter),
// sigma2, the latents resolved, SHO refused; no device work.  sparse_upload: x, y and z on the device, T = S^-1/2 U' and, on
// streams[0], the shard's rows of T y (Ty; sparse_core subtracts the means) with the regulariser's residual.
struct SparseTrain : Train {
  int d = 0, n = 0, p = 0, m = 0, nz = 0, with_regulariser = 0;
  const double *U = nullptr, *S = nullptr; double sigma2 = 0.0, jitter = 0.0;
  OilmmFront F{0, 0};
  Buf<double> z;                  // d x nz: the library's own copy (a posterior handle keeps it)
  const double* Ty = nullptr;     // [latent of the shard][n], in F
  double resid = 0.0, reg = 0.0;  // the copy queued by F.rows lands in resid; reg: sparse_value
};
static int sparse_resolve(bool bad, const double* x, int d, int n, const double* y, int p, const double* U, const double* S, int m, double sigma2,
                          const lmm_gp_t* gps, int l0, int l1, const double* z, int nz, double jitter, int with_regulariser, SparseTrain& T) {
  bad = bad || !x || !y || !U || !S || !z || d <= 0 || n <= 0 || p <= 0 || m <= 0 || nz <= 0;
  if (int rc = train_args(bad, p, m, S, sigma2, l0, l1, 0)) return rc;
  if (int rc = sparse_shape_check(d, nz, jitter)) return rc;
  if (!(sigma2 > 0.0)) return fail(LMM_ERR_ARG, "sigma2 must be > 0");
  if (int rc = train_resolve(gps, m, d, l0, l1, T)) return rc;
  T.d = d; T.n = n; T.p = p; T.m = m; T.nz = nz; T.with_regulariser = with_regulariser;
  T.U = U; T.S = S; T.sigma2 = sigma2; T.jitter = jitter;
  return refuse_sho(*T.ls, "inducing-point inference is");
}
static void sparse_upload(const double* x, const double* y, const double* z, SparseTrain& T) {
  hipStream_t st0 = g.streams[0];
  T.F = OilmmFront(T.U, T.S, T.p, T.m, T.sigma2);
  T.upload(x, (size_t)T.d * T.n, y, (size_t)T.n * T.p);
  T.z = Buf<double>((size_t)T.d * T.nz);
  HIPCHK(hipMemcpyAsync(T.z.p, z, (size_t)T.d * T.nz * sizeof(double), hipMemcpyDefault, st0));
  T.F.Td = Uploaded(T.F.T, st0);
  // (T y) of every latent when the regulariser needs the residual, else of the shard
  T.Ty = T.F.rows(T.yd.p, T.n, T.l0, T.ms, T.with_regulariser != 0, &T.resid);
}

// The value: sparse_core on the front end's rows (out.keep_grad: the gradient's inputs stay in `out`), streams[0] drained, and the
// regulariser of lmm_oilmm_logpdf in T.reg.
static int sparse_value(SparseTrain& T, SparseState& out) {
  hipStream_t st0 = g.streams[0];
  if (int rc = sparse_core(T.xd.p, T.d, T.n, T.z.p, T.nz, T.jitter, T.lts, T.l0, T.l1, T.Ty, T.means.data(), T.F.ST.data(), out)) {
    (void)hipStreamSynchronize(st0);      // the residual's copy targets T
    return rc;
  }
  HIPCHK(hipStreamSynchronize(st0));
  T.reg = T.with_regulariser ? oilmm_regulariser(T.n, T.p, T.m, T.S, T.sigma2, T.resid) : 0.0;
  return LMM_OK;
}

// The gradient of the bound from the value's factors (`out`, kept with keep_grad): the second pass over the points, the latents' own
// gradients (grad_finish with the K_uu diagonal and the kappa term in [7]), then the complete-data back end with d elbo_l / d r in the
// place of -alpha and d elbo_l / d w in the place of d lml / d noise.  gy_dev (n x p), gz_dev (d x nz): device outputs or nullptr.
static int sparse_oilmm_grad(const SparseTrain& T, const SparseState& out, OilmmGrad& G, double* gy_dev, double* gz_dev) {
  hipStream_t st0 = g.streams[0];
  const int d = T.d, n = T.n, l0 = T.l0, l1 = T.l1, ms = T.ms, mk = T.mk, NGR = LMM_NGRAD;
  const Latent* lts = T.lts;
  std::vector<double> hred, hard, gksum;
  Buf<double> gr((size_t)n * mk);
  if (int rc = sparse_grad_core(T.xd.p, d, n, T.z.p, T.nz, T.ls.get(), l0, l1, T.Ty, T.means.data(), T.F.ST.data(), out, hred, hard, gksum, gr.p,
                                gz_dev)) return rc;
  std::vector<double> dw(mk, 0.0);
  OilmmGradIn in{T.yd.p, n, T.p, T.U, T.S, T.m, one_noise_block(n, T.sigma2), l0, l1, T.with_regulariser};
  in.a = gr.p; in.lda = n; in.sgn = -1.0; in.dot = T.Ty; in.want_sum = true;      // sum_t d elbo_l / d r_t: minus the mean's gradient
  OilmmGradBackEnd B(in);
  HIPCHK(hipStreamSynchronize(st0));
  const std::vector<int> toff = T.ls->term_offsets(l0, l1);
  G.size(T.m, T.p, 1, d);
  for (int k = 0; k < ms; ++k) {
    const int l = l0 + k;
    const double w = T.F.ST[l];
    double* r = &hred[(size_t)NGR * toff[k]];
    const double gk = gksum[k];                          // sum_{i,t} g_it k_it = 2 tr(PhiBar Phi) + beta'b
    const double trK = -0.5 * r[1];                      // tr KuuBar
    dw[k] = -(0.5 * gk + 0.5 * out.ctc[k] - 0.5 * out.s[k] - 0.5 * out.kappa[k]) / w - (double)n / (2.0 * w);
    // [7] of a term: + the diagonal of K_uu and the kappa term, both linear in V_c
    for (int c = 0; c < lts[l].nt(); ++c) r[NGR * c + 7] += lts[l].terms[c].ev.var * (trK - 0.5 * (double)n / w);
    double dv0 = 0.0;
    G.ggps[l].lengthscale = grad_finish(lts[l], d, r, &hard[(size_t)d * toff[k]], 0.0, 0.0,
                                        &G.trec[(size_t)l * LMM_SUM_MAX_TERMS * term_grad_stride(d)], &dv0);
    G.ggps[l].variance = dv0;
    G.ggps[l].mean = -B.asum[k];
  }
  G.value = T.reg;                                       // the sum of lmm_oilmm_elbo, in its order
  for (int k = 0; k < ms; ++k) G.value += out.elbo[k];
  double reg_value = 0.0;                                // (the regulariser's value is T.reg)
  B.finish(dw.data(), nullptr, T.F.T, reg_value, G, gy_dev);
  return LMM_OK;
}

// elbo(VFE(f(z, jitter)), fx, y) and dtc(...) of AbstractGPs (src/sparse_approximations.jl) on the latents of an OILMM after the
// projection of reference src/oilmm.jl:79-93: *elbo = sum_{l in shard} elbo_l + (with_regulariser ? reg : 0), *dtc likewise.
int lmm_oilmm_elbo(const double* x, int d, int n, const double* y, int p, const double* U, const double* S, int m, double sigma2,
                   const lmm_gp_t* gps, int latent_begin, int latent_end, const double* z, int nz, double jitter,
                   int with_regulariser, double* elbo, double* dtc) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  SparseTrain T;
  if (int rc = sparse_resolve(!elbo && !dtc, x, d, n, y, p, U, S, m, sigma2, gps, latent_begin, latent_end, z, nz, jitter, with_regulariser, T))
    return rc;
  sparse_upload(x, y, z, T);
  SparseState st;
  if (int rc = sparse_value(T, st)) return rc;
  double e = T.reg, t = T.reg;
  for (size_t k = 0; k < st.elbo.size(); ++k) { e += st.elbo[k]; t += st.dtc[k]; }
  if (elbo) *elbo = e;
  if (dtc) *dtc = t;
  return LMM_OK;
  LMM_CATCH
}

// Value and gradient of elbo(VFE(f(z, jitter)), fx, y) with respect to y, sigma2, S, U, every latent's kernel parameters and mean (as
// lmm_oilmm_logpdf_grad returns them: grad_gps and the tag registry) and the inducing inputs z.  *out_elbo is bitwise the value of
// lmm_oilmm_elbo.  Any output may be NULL.
int lmm_oilmm_elbo_grad(const double* x, int d, int n, const double* y, int p, const double* U, const double* S, int m, double sigma2,
                        const lmm_gp_t* gps, int latent_begin, int latent_end, const double* z, int nz, double jitter,
                        int with_regulariser, double* out_elbo, double* grad_y, double* grad_sigma2, double* grad_S, double* grad_U,
                        lmm_gp_grad_t* grad_gps, double* grad_z) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  // its own arguments and the shape are reported ahead of the front end's m > p and shard (the pinned order), the ARD width after it
  if (!x || !y || !U || !S || !z || d <= 0 || n <= 0 || p <= 0 || m <= 0 || nz <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  if (int rc = sparse_shape_check(d, nz, jitter)) return rc;
  hipStream_t st0 = g.streams[0];
  DevOut gy(grad_y, (size_t)n * p), gz(grad_z, (size_t)d * nz);
  SparseTrain T;
  if (int rc = sparse_resolve(false, x, d, n, y, p, U, S, m, sigma2, gps, latent_begin, latent_end, z, nz, jitter, with_regulariser, T)) return rc;
  if (int rc = T.ls->ard_grad_check()) return rc;
  sparse_upload(x, y, z, T);
  SparseState st;
  st.keep_grad = true;
  if (int rc = sparse_value(T, st)) return rc;
  OilmmGrad G;
  if (int rc = sparse_oilmm_grad(T, st, G, gy.p, gz.p)) return rc;
  write_oilmm_grad(G, out_elbo, grad_sigma2, grad_S, grad_U, grad_gps);
  publish_grads(*T.ls, grad_gps ? &G.trec : nullptr, latent_begin, latent_end);
  if (grad_y) gy.finish(st0);
  if (grad_z) gz.finish(st0);
  if (grad_y || grad_z) HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

// posterior(VFE(f(z, jitter)), fx, y) of AbstractGPs (ApproxPosteriorGP) per latent of the shard: keeps z, L_u, L_B and c.
int lmm_oilmm_sparse_posterior_create(const double* x, int d, int n, const double* y, int p, const double* U, const double* S, int m,
                                      double sigma2, const lmm_gp_t* gps, int latent_begin, int latent_end, const double* z, int nz,
                                      double jitter, lmm_sparse_post_t** out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  SparseTrain T;
  if (int rc = sparse_resolve(!out, x, d, n, y, p, U, S, m, sigma2, gps, latent_begin, latent_end, z, nz, jitter, 0, T)) return rc;
  sparse_upload(x, y, z, T);
  SparseState st;
  if (int rc = sparse_value(T, st)) return rc;
  auto P = std::make_unique<lmm_sparse_post>();
  Dims D(nz, 1);
  P->d = d; P->nz = nz; P->l0 = latent_begin; P->l1 = latent_end; P->m = m; P->NC = D.NC; P->NR = D.NR; P->ld = D.ld;
  P->ls = T.ls; P->z = std::move(T.z);
  P->Lu = std::move(st.Lu); P->Wu = std::move(st.Wu); P->LB = std::move(st.LB); P->WB = std::move(st.WB); P->c = std::move(st.c);
  *out = P.release();
  return LMM_OK;
  LMM_CATCH
}

int lmm_sparse_post_destroy(lmm_sparse_post_t* post) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (post) {
    if (post->magic != LMM_SPARSE_POST_MAGIC) return fail(LMM_ERR_ARG, "not a handle of lmm_oilmm_sparse_posterior_create");
    if (g.init) (void)hipDeviceSynchronize();
    post->magic = 0;
    delete post;
  }
  return LMM_OK;
}

// mean_and_var(post(xs, sigma2)) of the ApproxPosteriorGP latents, mixed as lmm_oilmm_mean_and_var mixes exact ones (reference
// src/oilmm.jl:57-76).  Per latent, with a = L_u^-1 k_u(x*): mean = mean_l + (L_B^-1 a)' c, var = k** - |a|^2 + |L_B^-1 a|^2.
// gps is not read (the handle keeps its latents).  Outputs: the shard's partial sums, ns * p, by outputs; var may be NULL.
int lmm_oilmm_sparse_mean_and_var(const lmm_sparse_post_t* post, const lmm_gp_t* gps, const double* U, const double* S, int p, int m,
                                  double sigma2, int add_noise, const double* xs, int d, int ns, double* mean_out, double* var_out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  (void)gps;
  if (!post || !U || !S || !xs || !mean_out || d <= 0 || ns <= 0 || p <= 0 || m <= 0) return fail(LMM_ERR_ARG, "bad arguments");
  if (g_f32) return fail(LMM_ERR_UNSUPPORTED, "inducing-point inference is Float64 only (lmm_set_compute_dtype(LMM_F64))");
  if (post->magic != LMM_SPARSE_POST_MAGIC) return fail(LMM_ERR_ARG, "not a handle of lmm_oilmm_sparse_posterior_create");
  if (post->m != m) return fail(LMM_ERR_DIM, "posterior has %d latents, H has %d", post->m, m);
  if (post->d != d) return fail(LMM_ERR_DIM, "input dimension mismatch: posterior has d=%d, xs has d=%d", post->d, d);
  const lmm_sparse_post* P = post;
  const int l0 = P->l0, l1 = P->l1, ms = l1 - l0, M = P->nz;
  hipStream_t st0 = g.streams[0];
  const std::vector<double> Hs = shard_H(U, S, p, l0, ms);
  Uploaded Hd(Hs, st0);
  DevIn xsd(xs, (size_t)d * ns, st0);
  Buf<double> ml((size_t)ns * std::max(ms, 1)), vl((size_t)ns * std::max(ms, 1)), v1(ns), v2(ns), tmp(ns);
  const int nsr = rup(ns, 64);
  const int ldr = pad_ld(nsr);
  Buf<double> R((size_t)ldr * P->NC), part(strip_partial_elems(nsr, P->NC, 2));
  for (int k = 0; k < ms; ++k) {
    const Latent& gp = P->ls->lat[l0 + k];
    GramArgs r{};      // R (nsr x NC, ldr) = K(xs, z) as rider rows, rows beyond ns zero
    r.A = R.p; r.ld = ldr; r.nrows = P->NC + nsr; r.ncols = P->NC; r.row_tile0 = P->NC / 64; r.row_shift = P->NC; r.full = 1;
    r.x = P->z.p; r.d = d; r.n = M; gp.set_kernel(r);
    r.xs = xsd.p; r.ns = ns;
    gram_g(r, st0, "inducing cross-Gram assembly");
    BatchPtr Rb{}, Lub{}, Wub{}, LBb{}, WBb{};
    Rb.p[0] = R.p; Lub.p[0] = P->Lu[k].p; Wub.p[0] = P->Wu[k].p; LBb.p[0] = P->LB[k].p; WBb.p[0] = P->WB[k].p;
    trsm_rec(Rb, ldr, nsr, Lub, P->ld, Wub, 1, 0, P->NC, st0, false, true, true);      // rows a' = k_u(x*)' L_u^-T (no split-K atomics)
    rider_stats_g(R.p, ldr, ns, M, P->c[k].p, 0.0, gp.prior_var(), part.p, tmp.p, v1.p, st0);      // v1 = k** - |a|^2
    trsm_rec(Rb, ldr, nsr, LBb, P->ld, WBb, 1, 0, P->NC, st0, false, true, true);      // rows (L_B^-1 a)'
    rider_stats_g(R.p, ldr, ns, M, P->c[k].p, gp.mean, 0.0, part.p, ml.p + (size_t)k * ns, v2.p, st0);   // v2 = -|L_B^-1 a|^2
    launch_vec_lin(v1.p, v2.p, -1.0, ns, vl.p + (size_t)k * ns, st0);
  }
  DevOut mo(mean_out, (size_t)ns * p), vo(var_out, (size_t)ns * p);
  mix_marginals(ml.p, ns, ms, Hd.buf.p, p, 1, 0.0, 0.0, mo.p, st0);
  if (var_out) mix_marginals(vl.p, ns, ms, Hd.buf.p, p, 2, kDefaultJit.default_jitter, add_noise ? sigma2 : 0.0, vo.p, st0);
  mo.finish(st0); vo.finish(st0);
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

// Building block for tests: the moments of ONE latent from device pointers.  Phi: nz x nz column-major (ld), only its lower triangle
// is written; b: nz; scalars: s, kappa, lambda.  chunk: points per partial (0: the library's default).
int lmm_dev_sparse_moments(const double* x, int d, int n, const double* z, int nz, const lmm_gp_t* gp, const double* w, const double* r,
                           int chunk, double* Phi, int ld, double* b, double* scalars) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!x || !z || !gp || !w || !r || !Phi || !b || !scalars || d <= 0 || n <= 0 || nz <= 0 || ld < nz) return fail(LMM_ERR_ARG, "bad arguments");
  if (int rc = sparse_size_check(d, nz)) return rc;
  RESOLVE(gp, 1, d);
  if (int rc = refuse_sho(*ls, "inducing-point inference is")) return rc;
  int nch = 0;
  if (int rc = sparse_plan(n, nz, 1, chunk, &chunk, &nch)) return rc;
  hipStream_t st0 = g.streams[0];
  Buf<double> scratch((size_t)nch * sparse_partial_stride(nz));
  SparseMomArgs a{};
  sparse_fill_lat(a.lat[0], lts[0], w, 0.0, r, 0.0);
  BatchPtr Pb{}, bb{}, sb{};
  Pb.p[0] = Phi; bb.p[0] = b; sb.p[0] = scalars;
  sparse_moments_pass(a, SparsePoints{x, d, n, z, nz, chunk, nch}, scratch.p, 1, sum_mode(lts, 0, 1), Pb, ld, false, bb, sb, st0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

// Building block for tests: the second pass over the points for ONE latent from device pointers (sparse_grad_kernel and its finish).
// PhiBar: nz x nz column-major (ld), symmetric, both triangles; beta: nz.  term_records: LMM_SUM_MAX_TERMS records of LMM_NGRAD + d raw
// sums of the K_uf pass ([0] d/d multiplier, [7] sum g k_c, [8] alpha or rho, [9] decay, then the d per-dimension sums; zeros elsewhere and
// for the terms the latent does not have); grad_z: sum_t g_it d k / d z_i (d x nz); grad_r: (beta' k_t - r_t) / w_t (n).
int lmm_dev_sparse_grad(const double* x, int d, int n, const double* z, int nz, const lmm_gp_t* gp, const double* w, const double* r,
                        const double* PhiBar, int ld, const double* beta, int chunk, double* term_records, double* grad_z,
                        double* grad_r) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!x || !z || !gp || !w || !r || !PhiBar || !beta || !term_records || d <= 0 || n <= 0 || nz <= 0 || ld < nz)
    return fail(LMM_ERR_ARG, "bad arguments");
  if (int rc = sparse_size_check(d, nz)) return rc;
  RESOLVE(gp, 1, d);
  if (int rc = refuse_sho(*ls, "inducing-point inference is")) return rc;
  int nch = 0;
  if (int rc = sparse_plan(n, nz, 1, chunk, &chunk, &nch)) return rc;
  hipStream_t st0 = g.streams[0];
  const int tm = (nz + 63) / 64;
  Buf<double> scratch((size_t)nch * tm * sparse_grad_partial_stride(d));
  std::vector<LatentDev> hgd;
  for (const KernelTerm& T : lts[0].terms) hgd.push_back(T.gd);
  Buf<LatentDev> gdd(hgd.size());
  HIPCHK(hipMemcpyAsync(gdd.p, hgd.data(), hgd.size() * sizeof(LatentDev), hipMemcpyHostToDevice, st0));
  SparseGradLat hl{};
  sparse_grad_fill_lat(hl, lts[0], gdd.p, w, 0.0, r, 0.0, PhiBar, beta, grad_r);
  Buf<SparseGradLat> dl(1);
  BatchPtr rb{}, zb{};
  rb.p[0] = term_records; zb.p[0] = grad_z;
  sparse_grad_pass(&hl, dl.p, SparsePoints{x, d, n, z, nz, chunk, nch}, ld, scratch.p, 1, sum_mode(lts, 0, 1), rb, zb, st0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

}  // extern "C": the entry points below have C linkage from their declarations in include/lmm_hip.h

// ------------------------------------------------------------------------------------------------
// State-space inference for Matern12 / 32 / 52 and SHO latents over a one-dimensional input (include/lmm_hip.h "state space"):
// the Kalman filter and the RTS smoother as parallel scans over the points (lmm_kernels_ss.hip), linear in n and exact.
// ------------------------------------------------------------------------------------------------
#define LMM_SS_BATCH_BYTES (size_t(1) << 30)       // device memory one launch's latents may take (aggregates, filtered states)

// The model of a latent's launches (lmm_internal.h): that of its kind, or of the sum of its two terms (*swapped: the second term comes
// first in the library's order of the terms); 0: not served.  A term is served as a plain latent is: no factors, a tag only for an SHO
// term's quality.
static int ss_latent_model(const Latent& L, int* swapped = nullptr) {
  if (swapped) *swapped = 0;
  for (const KernelTerm& T : L.terms)
    if (T.has_ard || T.ev.ils != nullptr || (T.tag != 0 && T.ev.kind != LMM_KERNEL_SHO)) return 0;
  if (!L.is_sum()) return L.nt() == 1 ? ss_model_of(L.kind) : 0;
  return L.nt() == 2 ? ss_pair_model(ss_model_of(L.terms[0].ev.kind), ss_model_of(L.terms[1].ev.kind), swapped) : 0;
}
static int ss_latent_dim(const Latent& L) { return ss_model_dim(ss_latent_model(L)); }

// Every latent must be a plain Matern12 / 32 / 52 (no tag: per-dimension factors) or an SHO latent (whose tag, if any, carries its
// quality: resolve has checked it), or the sum of two such terms with a state dimension of at most 4 (DESIGN.md 4.18 "Sum latents").
// Names the first that is not.  refuse_sums: the entry point serves no sum latent (the gradients with respect to locations).
static int ss_check_latents(const Latent* lts, int m, bool refuse_sums = false) {
  for (int l = 0; l < m; ++l) {
    const Latent& L = lts[l];
    if (refuse_sums && L.is_sum()) {
      g.err_latent = l; g.err_info = 0;
      return fail(LMM_ERR_UNSUPPORTED, "latent %d: gradients with respect to locations are not served for a sum latent on the state-space path", l);
    }
    if (ss_latent_model(L) == 0) {
      g.err_latent = l; g.err_info = 0;
      // (the wording is pinned by tests from before SHO latents were admitted: it stays word for word)
      return fail(LMM_ERR_UNSUPPORTED, "state-space inference is served for plain Matern12, Matern32 and Matern52 latents: latent %d is not one", l);
    }
  }
  return LMM_OK;
}

static int ss_refuse_f32() { return fail(LMM_ERR_UNSUPPORTED, "state-space inference is Float64 only (lmm_set_compute_dtype(LMM_F64))"); }

// The first index a device check (launch_ss_sorted, launch_ss_finite) flags among the n values at xd, INT_MAX when it flags none: the
// flag goes up as INT_MAX, the kernel lowers it, the flag comes down.  A flagged index is left in the error detail's `info`.
static int ss_first_flagged(void (*launch)(const double*, int, int*, hipStream_t), const double* xd, int n) {
  hipStream_t st0 = g.streams[0];
  Buf<int> flag(1);
  int h = INT_MAX;
  HIPCHK(hipMemcpyAsync(flag.p, &h, sizeof(int), hipMemcpyHostToDevice, st0));
  launch(xd, n, flag.p, st0);
  HIPCHK(hipMemcpyAsync(&h, flag.p, sizeof(int), hipMemcpyDeviceToHost, st0));
  HIPCHK(hipStreamSynchronize(st0));
  if (h != INT_MAX) { g.err_latent = -1; g.err_info = h; }
  return h;
}
// x (device, n values) must be non-decreasing: LMM_ERR_ARG with the first offending index in the error detail's `info`.
static int ss_check_sorted(const double* xd, int n) {
  const int h = ss_first_flagged(launch_ss_sorted, xd, n);
  if (h == INT_MAX) return LMM_OK;
  return fail(LMM_ERR_ARG, "state-space inference needs non-decreasing inputs: x[%d] is not >= x[%d] (sort the points first)", h, h - 1);
}
// xs (device, ns values) must be finite: LMM_ERR_ARG with the first offending index in the error detail's `info`.
static int ss_check_finite(const double* xsd, int ns) {
  const int h = ss_first_flagged(launch_ss_finite, xsd, ns);
  if (h == INT_MAX) return LMM_OK;
  return fail(LMM_ERR_ARG, "state-space posterior: xs[%d] is not finite", h);
}

// The plan of a scan over n items: `chunk` items per thread (<= 0: the library's choice, a function of n alone) and the threads it takes
struct SSChunks { int chunk, nch; };
static SSChunks ss_plan_chunks(int n, int chunk) {
  if (chunk <= 0) chunk = ss_default_chunk(n);
  if (chunk > n) chunk = n;
  return SSChunks{chunk, (n + chunk - 1) / chunk};
}

// The launches of ne entries (latents, or (latent, sample) pairs), entry e belonging to latent lat_of(e): consecutive entries share a
// launch while their model is the same (ss_model_of: Matern32 and SHO share a state dimension, not a launch), up to LMM_MAX_BATCH and
// to the LMM_SS_BATCH_BYTES / bytes_per_entry(model, D, nch) entries whose buffers the launch may hold, and at least one.
// body(e0, nb, model, D) runs the launch of entries [e0, e0 + nb).
template <typename LatOf, typename Bytes, typename Body>
static void ss_for_launches(long long ne, int nch, LatOf&& lat_of, Bytes&& bytes_per_entry, Body&& body) {
  for (long long e0 = 0; e0 < ne;) {
    const int model = ss_latent_model(lat_of(e0)), D = ss_model_dim(model);
    const int nbmax = (int)std::max<size_t>(1, std::min<size_t>(LMM_MAX_BATCH, LMM_SS_BATCH_BYTES / bytes_per_entry(model, D, nch)));
    int nb = 1;
    while (e0 + nb < ne && nb < nbmax && ss_latent_model(lat_of(e0 + nb)) == model) ++nb;
    body(e0, nb, model, D);
    e0 += nb;
  }
}

// the kernel parameters every *Lat struct of a launch takes from its latent; a sum latent's terms go in the library's order, with the
// sum's own variance and lengthscale folded in (KernelTerm::ev) and an SHO term's quality from the alpha slot of its descriptor
template <typename Lat>
static void ss_fill_kernel(Lat& o, const Latent& L) {
  int sw = 0;
  ss_latent_model(L, &sw);
  const KernelTerm& A = L.terms[sw ? 1 : 0];
  o.var = A.ev.var; o.inv_ls = A.ev.inv_ls; o.quality = L.is_sum() ? A.ev.alpha : L.quality;
  o.var2 = 0.0; o.inv_ls2 = 0.0; o.quality2 = 0.0;
  if (L.is_sum()) {
    const KernelTerm& B = L.terms[sw ? 0 : 1];
    o.var2 = B.ev.var; o.inv_ls2 = B.ev.inv_ls; o.quality2 = B.ev.alpha;
  }
}
template <typename Lat>
static void ss_fill_lat(Lat& o, const Latent& L, bool add_mean) {
  ss_fill_kernel(o, L);
  o.mean = add_mean ? L.mean : 0.0;
}
#define SS_NTHETA 6                    // kernel parameters a latent's forward-mode gradient seeds at the most (an SHO + SHO sum: 3 + 3)

// The filter (and, smean != nullptr, the smoother) of the ms latents lts[0 .. ms): w, r, fmean, fvar, smean, svar are [latent][n] on
// the device (outputs may be nullptr); lml: ms host values or nullptr; add_mean: the smoothed means get the latent's mean added.
// Latents run in launches of one model (ss_model_of: Matern32 and SHO share a state dimension, not a launch), as many per launch as
// LMM_SS_BATCH_BYTES admits.  Returns with streams[0] drained.
// go != nullptr (with smean, svar and add_mean = false): the gradients of every latent's log density as well.
struct SSGradOut {
  double* alpha; double* grad_w;       // device, [latent][n]: alpha_t = -d lml / d r_t, d lml / d w_t
  double* sums;                        // host, 4 per latent: sum_t alpha_t, w_t alpha_t^2, w_t c_t, d lml / d w_t
  double* gtheta;                      // host, SS_NTHETA per latent: d lml / d variance, d lml / d lengthscale, d lml / d quality (SHO; else 0); a sum
                                       // latent: its first term's (in the library's order), then its second's, each with a quality only when SHO
  double* gdt = nullptr;               // device, [latent][n] (nullptr: not computed): d lml / d (x_t - x_{t-1}), 0 at t = 0
};
// One entry of the latent dimension of a launch: a latent with its own noise and data (n values each, on the device).  Samples ride
// through the filter and smoother as several entries of one latent, with the same w and their own r.
struct SSEntry { const Latent* L; const double* w; const double* r; };
// keep != nullptr: the filtered and the full smoothed states (zero-mean) of every entry go to the caller's buffers, entry k's
// n x ss_state_comps(D_k) block (point-major) ss_keep_offset(es, k, n) doubles in; the smoother runs whether or not smean is given.
struct SSKeep { double* fstate; double* sstate; };
static size_t ss_keep_offset(const SSEntry* es, int k, int n) {
  size_t off = 0;
  for (int j = 0; j < k; ++j) off += (size_t)ss_state_comps(ss_latent_dim(*es[j].L)) * n;
  return off;
}
static int ss_core_entries(const double* xd, int n, const SSEntry* es, int ms, int chunk, double* lml, double* fmean, double* fvar,
                           double* smean, double* svar, bool add_mean, const SSGradOut* go = nullptr, const SSKeep* keep = nullptr) {
  hipStream_t st0 = g.streams[0];
  const SSChunks plan = ss_plan_chunks(n, chunk);
  const int nch = plan.nch, npb = ss_point_blocks(n);
  const bool smooth = smean != nullptr || keep != nullptr;
  const auto bytes = [&](int model, int D, int nch) {       // a latent's aggregates, partials and filtered states
    const int NS = ss_model_seeds(model);
    return (ss_fwd_agg_elems(D, nch) + (size_t)nch + (smooth ? (size_t)ss_state_comps(D) * n + ss_bwd_agg_elems(D, nch) : 0) +
            (go ? ss_dual_agg_elems(D, nch, NS) + NS * (size_t)nch + 4 * (size_t)npb : 0)) * sizeof(double);
  };
  ss_for_launches(ms, nch, [&](long long k) -> const Latent& { return *es[k].L; }, bytes, [&](long long e0, int nb, int model, int D) {
    const int k0 = (int)e0, NS = ss_model_seeds(model);
    const size_t comps = (size_t)ss_state_comps(D);
    Buf<double> agg((size_t)nb * ss_fwd_agg_elems(D, nch)), part((size_t)nb * nch), lmld(nb), state, bagg;
    if (smooth) { state = Buf<double>((size_t)nb * comps * n); bagg = Buf<double>((size_t)nb * ss_bwd_agg_elems(D, nch)); }
    Buf<double> dagg, dpart, ppart, gsum;
    std::vector<double> gth((size_t)nb * NS);     // the launch's NS values per latent
    if (go) {
      dagg = Buf<double>((size_t)nb * ss_dual_agg_elems(D, nch, NS)); dpart = Buf<double>((size_t)nb * NS * nch);
      ppart = Buf<double>((size_t)nb * 4 * npb); gsum = Buf<double>((size_t)nb * (4 + NS));
    }
    SSArgs a{};
    a.x = xd; a.n = n; a.chunk = plan.chunk; a.nch = nch;
    a.agg = agg.p; a.bagg = bagg.p; a.part = part.p;
    a.fmean = fmean ? fmean + (size_t)k0 * n : nullptr; a.fvar = fvar ? fvar + (size_t)k0 * n : nullptr;
    a.state = state.p; a.state_stride = comps * n;
    if (keep) { const size_t off = ss_keep_offset(es, k0, n); a.fkeep = keep->fstate + off; a.sstate = keep->sstate + off; }
    a.smean = (smooth && smean) ? smean + (size_t)k0 * n : nullptr; a.svar = (smooth && svar) ? svar + (size_t)k0 * n : nullptr;
    a.dagg = dagg.p; a.dpart = dpart.p;
    a.gdt = (go && go->gdt) ? go->gdt + (size_t)k0 * n : nullptr;
    for (int j = 0; j < nb; ++j) {
      ss_fill_lat(a.lat[j], *es[k0 + j].L, add_mean);
      a.lat[j].w = es[k0 + j].w; a.lat[j].r = es[k0 + j].r;
    }
    launch_ss_filter(a, model, nb, lmld.p, st0);
    if (smooth) launch_ss_smooth(a, model, nb, st0);
    if (go) {
      launch_ss_point(a, nb, go->alpha + (size_t)k0 * n, go->grad_w + (size_t)k0 * n, ppart.p, gsum.p, st0);
      launch_ss_grad(a, model, nb, gsum.p + (size_t)nb * 4, st0);
    }
    HIPCHK(hipGetLastError());
    if (lml) HIPCHK(hipMemcpyAsync(lml + k0, lmld.p, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, st0));
    if (go) {
      HIPCHK(hipMemcpyAsync(go->sums + (size_t)k0 * 4, gsum.p, (size_t)nb * 4 * sizeof(double), hipMemcpyDeviceToHost, st0));
      HIPCHK(hipMemcpyAsync(gth.data(), gsum.p + (size_t)nb * 4, (size_t)nb * NS * sizeof(double), hipMemcpyDeviceToHost, st0));
    }
    HIPCHK(hipStreamSynchronize(st0));          // the buffers above go back to the pool
    if (go)
      for (int j = 0; j < nb; ++j)
        for (int s = 0; s < SS_NTHETA; ++s) go->gtheta[(size_t)(k0 + j) * SS_NTHETA + s] = s < NS ? gth[(size_t)j * NS + s] : 0.0;
  });
  return LMM_OK;
}

static int ss_core(const double* xd, int n, const Latent* lts, int ms, const double* w, const double* r, int chunk, double* lml,
                   double* fmean, double* fvar, double* smean, double* svar, bool add_mean, const SSGradOut* go = nullptr) {
  std::vector<SSEntry> es(ms);
  for (int k = 0; k < ms; ++k) es[k] = SSEntry{lts + k, w + (size_t)k * n, r + (size_t)k * n};
  return ss_core_entries(xd, n, es.data(), ms, chunk, lml, fmean, fvar, smean, svar, add_mean, go);
}

// The latents' kernel-parameter gradients from the forward-mode values gth (SS_NTHETA per latent of the shard [l0, l1), in the order of
// SSGradOut::gtheta): grad_gps[l] (m entries; nullptr: not wanted) gets d lml / d variance and d lml / d lengthscale, and the registry
// (publish_grads) an SHO latent's d lml / d quality (lmm_kernel_tag_quality_grad) and a sum latent's per-term values
// (lmm_kernel_sum_grad; an SHO term's quality through its own tag).  A sum's terms are V_c kappa_c(. / E_c) with V_c = v0 v_c and
// E_c = s0 l_c (an SHO term's period), which is what the kernels seed: d/dv_c = v0 d/dV_c, d/dl_c = s0 d/dE_c, d/dv0 = sum_c v_c d/dV_c
// and d/ds0 = sum_c l_c d/dE_c, the dense path's semantics (grad_finish).  gth == nullptr (grad_gps NULL): the tags are reset to zeros.
static void ss_publish_grads(const LatentSet& S, int l0, int l1, const double* gth, lmm_gp_grad_t* ggps) {
  if (!gth) { publish_grads(S, nullptr, l0, l1); return; }
  const size_t sw = term_grad_stride(S.d);
  std::vector<double> trec(S.lat.size() * LMM_SUM_MAX_TERMS * sw, 0.0);
  for (int l = l0; l < l1; ++l) {
    const Latent& L = S.lat[l];
    const double* gl = gth + (size_t)SS_NTHETA * (l - l0);
    double* rec = &trec[(size_t)l * LMM_SUM_MAX_TERMS * sw];
    if (!L.is_sum()) {
      if (ggps) { ggps[l].variance = gl[0]; ggps[l].lengthscale = gl[1]; }
      rec[0] = gl[0]; rec[1] = gl[1]; rec[2] = gl[2];
      continue;
    }
    int swapped = 0;
    const int model = ss_latent_model(L, &swapped);
    const int na = ss_model_seeds(model / SS_PAIR(1, 0));
    double dv0 = 0.0, ds0 = 0.0;
    for (int c = 0; c < 2; ++c) {
      const KernelTerm& T = L.terms[c];
      const double* gc = gl + ((c == 0) == (swapped == 0) ? 0 : na);      // the term's seeds: first in the library's order, or behind the first's
      double* o = rec + sw * c;
      o[0] = L.variance * gc[0]; o[1] = L.lengthscale * gc[1]; o[2] = T.ev.kind == LMM_KERNEL_SHO ? gc[2] : 0.0;
      dv0 += T.v * gc[0]; ds0 += T.ls * gc[1];
    }
    if (ggps) { ggps[l].variance = dv0; ggps[l].lengthscale = ds0; }
  }
  publish_grads(S, &trec, l0, l1);
}

// The OILMM front end of the state-space path: per latent of the shard and point, the pseudo-observation r = z_t[l] - mean_l and its
// noise variance w = sigma2 (G_t^-1)_ll of the missing-data projection (missing_front; without NaN that is (T y)_l - mean_l and
// sigma2 / S_l), with w = +Inf and r = 0 at the points without any observed output, which the front end itself never sees.
struct SSFront {
  Buf<double> w, r;        // [l1 - l0][n]
  double reg = 0.0;        // sum_t r_t over the points with observations
  // for the gradient: whether any entry of y is NaN, the points with observations (idx, on the device idxd; all n when nobs == n) and
  // the front end's state over those nobs points (its z and nv have moved into r and w when nobs == n)
  bool has_nan = false;
  int nobs = 0;
  std::vector<int> idx;
  Buf<int> idxd;
  MissingFront F;
};
static int ss_front(const double* yd, int n, int p, const double* U, const double* S, int m, double s2, const Latent* lts, int l0, int l1,
                    SSFront& Fr, bool want_resid = false, int point0 = 0) {      // point0: the caller's number of point 0 (an append: the handle's n)
  hipStream_t st0 = g.streams[0];
  const int nw = (p + 63) / 64, ms = l1 - l0;
  std::vector<int> hpt(n);
  std::vector<int>& idx = Fr.idx;
  MissingFront& F = Fr.F;
  {
    Buf<unsigned long long> masks((size_t)n * nw);
    Buf<int> pt(n);
    launch_missing_masks(yd, n, p, masks.p, pt.p, st0);
    HIPCHK(hipMemcpyAsync(hpt.data(), pt.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st0));
    HIPCHK(hipStreamSynchronize(st0));
  }
  for (int t = 0; t < n; ++t) {
    if (hpt[t] > 0 && hpt[t] < m) {
      g.err_latent = -1; g.err_info = point0 + t;
      return fail(LMM_ERR_UNSUPPORTED, "missing data: point %d observes %d outputs, fewer than the m = %d latent processes", point0 + t, hpt[t], m);
    }
    if (hpt[t] > 0) idx.push_back(t);
    if (hpt[t] != p) Fr.has_nan = true;
  }
  const int nobs = (int)idx.size();
  Fr.nobs = nobs;
  const std::vector<double> means = latent_means(lts, m);
  if (nobs == n) {
    if (int rc = missing_front(yd, n, p, U, S, m, s2, means.data(), l0, l1, want_resid, F)) return rc;
    Fr.w = std::move(F.nv); Fr.r = std::move(F.z);
    Fr.reg = F.reg(n, m, s2);
    return LMM_OK;
  }
  Fr.w = Buf<double>((size_t)n * std::max(ms, 1)); Fr.r = Buf<double>((size_t)n * std::max(ms, 1));
  for (int k = 0; k < ms; ++k) {
    launch_fill(Fr.w.p + (size_t)k * n, n, INFINITY, st0);
    launch_fill(Fr.r.p + (size_t)k * n, n, 0.0, st0);
  }
  if (nobs > 0) {
    Fr.idxd = Buf<int>(nobs);
    Buf<int>& idxd = Fr.idxd;
    Buf<double> yc((size_t)nobs * p);
    HIPCHK(hipMemcpyAsync(idxd.p, idx.data(), (size_t)nobs * sizeof(int), hipMemcpyHostToDevice, st0));
    launch_ss_gather_rows(yd, n, p, idxd.p, nobs, yc.p, st0);
    if (int rc = missing_front(yc.p, nobs, p, U, S, m, s2, means.data(), l0, l1, want_resid, F)) {
      if (rc == LMM_ERR_NOT_PD && g.err_info >= 0 && g.err_info < nobs) {      // the front end numbered the points it saw
        g.err_info = point0 + idx[g.err_info];
        return fail(LMM_ERR_NOT_PD, "PosDefException: H_t' H_t of point %d is not positive definite over its observed outputs", g.err_info);
      }
      return rc;
    }
    if (ms > 0) {
      launch_ss_scatter_rows(F.nv.p, n, ms, idxd.p, nobs, Fr.w.p, st0);
      launch_ss_scatter_rows(F.z.p, n, ms, idxd.p, nobs, Fr.r.p, st0);
    }
    Fr.reg = F.reg(nobs, m, s2);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st0));            // yc and the front end's compacted z and nv go back to the pool
  F.z = Buf<double>(); F.nv = Buf<double>();
  return LMM_OK;
}

// The preamble of the entry points that take training data, in the order the error codes are pinned in: the argument checks (missing:
// x, y where the entry point needs it, or an output of its own is NULL), the Float64-only refusal, after_args (the entry point's own
// checks, if any), then the latents resolved and checked, x and y on the device, x checked, the shard's bounds and, with y, the front end.
struct SSTrain {
  std::shared_ptr<LatentSet> ls;
  const Latent* lts = nullptr;         // all m latents
  DevIn xd{nullptr, 0, nullptr}, yd{nullptr, 0, nullptr};
  int l0 = 0, l1 = 0, ms = 0, mk = 1;  // the shard, its latents, max(ms, 1)
  SSFront Fr;                          // left empty without y
};
static int ss_train(bool missing, const double* x, int n, const double* y, int p, const double* U, const double* S, int m, double sigma2,
                    const lmm_gp_t* gps, int l0, int l1, SSTrain& T, bool want_resid = false, const std::function<int()>& after_args = nullptr,
                    bool refuse_sums = false) {
  if (int rc = train_args(missing || !x || !U || !S || n <= 0 || p <= 0 || m <= 0, p, m, S, sigma2, l0, l1, TRAIN_SIGMA2 | TRAIN_S)) return rc;
  if (g_f32) return ss_refuse_f32();
  if (after_args)
    if (int rc = after_args()) return rc;
  if (int rc = resolve(gps, m, 1, T.ls, true)) return rc;
  T.lts = T.ls->lat.data();
  if (int rc = ss_check_latents(T.lts, m, refuse_sums)) return rc;
  T.xd = DevIn(x, (size_t)n, g.streams[0]); T.yd = DevIn(y, (size_t)n * p, g.streams[0]);
  if (int rc = ss_check_sorted(T.xd.p, n)) return rc;
  T.l0 = l0; T.l1 = l1; T.ms = l1 - l0; T.mk = std::max(T.ms, 1);
  return y ? ss_front(T.yd.p, n, p, U, S, m, sigma2, T.lts, l0, l1, T.Fr, want_resid) : (int)LMM_OK;
}

int lmm_oilmm_logpdf_statespace(const double* x, int n, const double* y, int p, const double* U, const double* S, int m, double sigma2,
                                const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  SSTrain T;
  if (int rc = ss_train(!y || !out, x, n, y, p, U, S, m, sigma2, gps, latent_begin, latent_end, T)) return rc;
  std::vector<double> lml(T.mk, 0.0);
  if (int rc = ss_core(T.xd.p, n, T.lts + T.l0, T.ms, T.Fr.w.p, T.Fr.r.p, 0, lml.data(), nullptr, nullptr, nullptr, nullptr, false)) return rc;
  double total = 0.0;
  for (int k = 0; k < T.ms; ++k) total += lml[k];
  if (with_regulariser) total += T.Fr.reg;
  *out = total;
  return LMM_OK;
  LMM_CATCH
}

int lmm_oilmm_mean_and_var_statespace(const double* x, int n, const double* y, int p, const double* U, const double* S, int m,
                                      double sigma2, const lmm_gp_t* gps, int latent_begin, int latent_end, int add_noise,
                                      double* mean_out, double* var_out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  SSTrain T;
  if (int rc = ss_train(!y || !mean_out, x, n, y, p, U, S, m, sigma2, gps, latent_begin, latent_end, T)) return rc;
  hipStream_t st0 = g.streams[0];
  const int ms = T.ms;
  Buf<double> ml((size_t)n * T.mk), vl((size_t)n * T.mk);
  if (int rc = ss_core(T.xd.p, n, T.lts + T.l0, ms, T.Fr.w.p, T.Fr.r.p, 0, nullptr, nullptr, nullptr, ml.p, vl.p, true)) return rc;
  Uploaded Hd(shard_H(U, S, p, T.l0, ms), st0);
  DevOut mo(mean_out, (size_t)n * p), vo(var_out, (size_t)n * p);
  // the mixing of lmm_oilmm_mean_and_var (reference src/oilmm.jl:69,72)
  mix_marginals(ml.p, n, ms, Hd.buf.p, p, 1, 0.0, 0.0, mo.p, st0);
  if (var_out) mix_marginals(vl.p, n, ms, Hd.buf.p, p, 2, kDefaultJit.default_jitter, add_noise ? sigma2 : 0.0, vo.p, st0);
  mo.finish(st0); vo.finish(st0);
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

// Value and gradient of lmm_oilmm_logpdf_statespace with respect to y, sigma2, S, U and every latent's (variance, lengthscale, mean), in
// O(n).  Per latent the smoother gives d lml / d r_t = -alpha_t and d lml / d w_t = (alpha_t^2 - c_t) / 2, and the
// forward-mode pass d lml / d variance and d lml / d lengthscale (ss_core with SSGradOut); the front end's chain rule is that of
// lmm_oilmm_elbo_grad for complete data and that of oilmm_grad_missing_core for data with NaN (then without S and U).  *out_logpdf is
// the sum of lmm_oilmm_logpdf_statespace in its order.  Partial sums over the shard; any output may be NULL.
// grad_x (lmm_oilmm_logpdf_grad_statespace_x; n values in the order of x, host or device; may be nullptr): the smoother's launches also
// write every spacing's d lml_l / d dt (SSGradOut::gdt), and launch_ss_grad_x adds the latents' d lml_l / d x_t = g_t - g_{t+1} in
// latent order.  The regulariser and the projection do not depend on x.
static int ss_logpdf_grad(const double* x, int n, const double* y, int p, const double* U, const double* S, int m, double sigma2,
                          const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser, double* out_logpdf, double* grad_y,
                          double* grad_sigma2, double* grad_S, double* grad_U, lmm_gp_grad_t* grad_gps, double* grad_x) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  SSTrain T;
  if (int rc = ss_train(!y, x, n, y, p, U, S, m, sigma2, gps, latent_begin, latent_end, T, grad_y && with_regulariser, nullptr, grad_x != nullptr)) return rc;
  hipStream_t st0 = g.streams[0];
  const auto& [ls, lts, xd, yd, l0, l1, ms, msa, Fr] = T;
  if (Fr.has_nan && (grad_S || grad_U))
    return fail(LMM_ERR_UNSUPPORTED, "state-space gradients with respect to S and U are not built for data with NaN (pass NULL for grad_S and grad_U)");
  DevOut gy(grad_y, (size_t)n * p);
  std::vector<double> lml(msa, 0.0), sums(4 * (size_t)msa, 0.0), gth(SS_NTHETA * (size_t)msa, 0.0);
  Buf<double> sm((size_t)n * msa), sv((size_t)n * msa), al((size_t)n * msa), gw((size_t)n * msa);
  DevOut gx(grad_x, (size_t)n);
  Buf<double> gd;
  if (grad_x) gd = Buf<double>((size_t)n * msa);
  const SSGradOut go{al.p, gw.p, sums.data(), gth.data(), gd.p};
  if (int rc = ss_core(xd.p, n, lts + l0, ms, Fr.w.p, Fr.r.p, 0, lml.data(), nullptr, nullptr, sm.p, sv.p, false, &go)) return rc;
  if (grad_x) {
    launch_ss_grad_x(gd.p, Fr.w.p, n, ms, gx.p, st0);
    HIPCHK(hipGetLastError());
    gx.finish(st0);
    HIPCHK(hipStreamSynchronize(st0));
  }
  double total = 0.0;
  for (int k = 0; k < ms; ++k) total += lml[k];
  if (with_regulariser) total += Fr.reg;
  OilmmGrad G;
  G.size(m, p, 1, 1);
  G.value = total;
  for (int k = 0; k < ms; ++k) G.ggps[l0 + k].mean = sums[4 * (size_t)k];      // sum_t alpha_t
  if (Fr.has_nan) {
    const MissingFront& F = Fr.F;
    const int nobs = Fr.nobs;
    // w_t = sigma2 (G_t^-1)_ll: sum_t (d lml / d w_t) w_t / sigma2, as oilmm_grad_missing_core
    for (int k = 0; k < ms; ++k) G.gs2[0] += 0.5 * (sums[4 * (size_t)k + 1] - sums[4 * (size_t)k + 2]) / sigma2;
    if (nobs == n) {
      missing_grad_back_end(F, n, p, m, sigma2, with_regulariser, al.p, n, l0, ms, G, gy.p);
    } else {
      // the front end numbered the nobs points with observations: alpha in that numbering, the rows of grad_y scattered back
      if (grad_y) for (int o = 0; o < p; ++o) launch_fill(gy.p + (size_t)o * n, n, 0.0, st0);
      if (nobs > 0) {
        Buf<double> ac, gyc;
        if (grad_y) {
          ac = Buf<double>((size_t)nobs * msa); gyc = Buf<double>((size_t)nobs * p);
          if (ms > 0) launch_ss_gather_rows(al.p, n, ms, Fr.idxd.p, nobs, ac.p, st0);
        }
        missing_grad_back_end(F, nobs, p, m, sigma2, with_regulariser, ac.p, nobs, l0, ms, G, gyc.p);
        if (grad_y) {
          launch_ss_scatter_rows(gyc.p, n, p, Fr.idxd.p, nobs, gy.p, st0);
          HIPCHK(hipGetLastError());
          HIPCHK(hipStreamSynchronize(st0));      // ac and gyc go back to the pool
        }
      }
    }
  } else {
    // complete data: r = (T y)_l - mean_l with T = S^-1/2 U' and w = sigma2 / S_l.  alpha = -d lml / d r is dotted with r, so the back
    // end adds mean_l * sum_t alpha_t; the regulariser's value is in G.value already (Fr.reg)
    std::vector<double> T, ST, H, dw(msa, 0.0), mean_sum(msa, 0.0);
    project_orthogonal(U, S, p, m, sigma2, T, ST, H);
    OilmmGradIn in{yd.p, n, p, U, S, m, one_noise_block(n, sigma2), l0, l1, with_regulariser};
    in.a = al.p; in.lda = n; in.dot = Fr.r.p;
    OilmmGradBackEnd B(in);
    HIPCHK(hipStreamSynchronize(st0));
    for (int k = 0; k < ms; ++k) {
      dw[k] = sums[4 * (size_t)k + 3];                                      // sum_t d lml / d w_t
      mean_sum[k] = lts[l0 + k].mean * sums[4 * (size_t)k];
    }
    double reg_value = 0.0;
    B.finish(dw.data(), mean_sum.data(), T, reg_value, G, gy.p);
    if (grad_y) HIPCHK(hipGetLastError());
  }
  ss_publish_grads(*ls, l0, l1, grad_gps ? gth.data() : nullptr, G.ggps.data());
  write_oilmm_grad(G, out_logpdf, grad_sigma2, grad_S, grad_U, grad_gps);
  if (grad_y) { gy.finish(st0); HIPCHK(hipStreamSynchronize(st0)); }
  return LMM_OK;
  LMM_CATCH
}

int lmm_oilmm_logpdf_grad_statespace(const double* x, int n, const double* y, int p, const double* U, const double* S, int m,
                                     double sigma2, const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser,
                                     double* out_logpdf, double* grad_y, double* grad_sigma2, double* grad_S, double* grad_U,
                                     lmm_gp_grad_t* grad_gps) {
  return ss_logpdf_grad(x, n, y, p, U, S, m, sigma2, gps, latent_begin, latent_end, with_regulariser, out_logpdf, grad_y, grad_sigma2,
                        grad_S, grad_U, grad_gps, nullptr);
}

int lmm_oilmm_logpdf_grad_statespace_x(const double* x, int n, const double* y, int p, const double* U, const double* S, int m,
                                       double sigma2, const lmm_gp_t* gps, int latent_begin, int latent_end, int with_regulariser,
                                       double* out_logpdf, double* grad_y, double* grad_sigma2, double* grad_S, double* grad_U,
                                       lmm_gp_grad_t* grad_gps, double* grad_x) {
  return ss_logpdf_grad(x, n, y, p, U, S, m, sigma2, gps, latent_begin, latent_end, with_regulariser, out_logpdf, grad_y, grad_sigma2,
                        grad_S, grad_U, grad_gps, grad_x);
}

// Building blocks for tests: ONE latent from device pointers, per-point noise w (+Inf: unobserved) and data r; the latent's mean is
// not read (r is the residual).  chunk: points per thread (0: the library's plan).
// The preamble of these one-latent entry points: `bad` (a NULL pointer or a size out of range) refuses the arguments, then nsamples
// (given by the entry points that draw samples), the Float64-only refusal, the latent resolved and checked, x (device) checked.
static int ss_dev_prepare(bool bad, const double* x, int n, const lmm_gp_t* gp, std::shared_ptr<LatentSet>& ls, int nsamples = 1,
                          bool refuse_sums = false) {
  if (bad) return fail(LMM_ERR_ARG, "bad arguments");
  if (nsamples < 1) return fail(LMM_ERR_ARG, "nsamples must be >= 1 (nsamples = %d)", nsamples);
  if (g_f32) return ss_refuse_f32();
  if (int rc = resolve(gp, 1, 1, ls, true)) return rc;
  if (int rc = ss_check_latents(ls->lat.data(), 1, refuse_sums)) return rc;
  return ss_check_sorted(x, n);
}

static int ss_dev_block(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, int chunk, double* fmean,
                        double* fvar, double* lml_dev, double* smean, double* svar) {
  std::shared_ptr<LatentSet> ls;
  if (int rc = ss_dev_prepare(n <= 0 || chunk < 0, x, n, gp, ls)) return rc;
  const Latent* lts = ls->lat.data();
  double lml = 0.0;
  if (int rc = ss_core(x, n, lts, 1, w, r, chunk, &lml, fmean, fvar, smean, svar, false)) return rc;
  if (lml_dev) {
    HIPCHK(hipMemcpyAsync(lml_dev, &lml, sizeof(double), hipMemcpyHostToDevice, g.streams[0]));
    HIPCHK(hipStreamSynchronize(g.streams[0]));
  }
  return LMM_OK;
}

int lmm_dev_statespace_filter(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, int chunk, double* fmean,
                              double* fvar, double* lml) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!x || !gp || !w || !r || !fmean || !fvar || !lml) return fail(LMM_ERR_ARG, "bad arguments");
  return ss_dev_block(x, n, gp, w, r, chunk, fmean, fvar, lml, nullptr, nullptr);
  LMM_CATCH
}

int lmm_dev_statespace_smooth(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, int chunk, double* smean,
                              double* svar) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!x || !gp || !w || !r || !smean || !svar) return fail(LMM_ERR_ARG, "bad arguments");
  return ss_dev_block(x, n, gp, w, r, chunk, nullptr, nullptr, nullptr, smean, svar);
  LMM_CATCH
}

// Building block for tests beside lmm_dev_statespace_filter: lml as there, grad_r and grad_w (n values each) and grad_theta =
// {d lml / d variance, d lml / d lengthscale} (ntheta = 2) or those and d lml / d quality (ntheta = 3), all on the device.
static int ss_dev_grad(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, int chunk, double* lml,
                       double* grad_r, double* grad_w, double* grad_theta, int ntheta) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  std::shared_ptr<LatentSet> ls;
  const bool bad = !x || !gp || !w || !r || !lml || !grad_r || !grad_w || !grad_theta || n <= 0 || chunk < 0;
  if (int rc = ss_dev_prepare(bad, x, n, gp, ls)) return rc;
  const Latent* lts = ls->lat.data();
  if (lts[0].is_sum() && ntheta < SS_NTHETA) {      // two or three values cannot carry a sum's seeds: lmm_dev_statespace_grad_sum does
    g.err_latent = 0; g.err_info = 0;
    return fail(LMM_ERR_UNSUPPORTED, "latent 0: a sum latent's gradient has up to %d kernel parameters (lmm_dev_statespace_grad_sum)", SS_NTHETA);
  }
  hipStream_t st0 = g.streams[0];
  Buf<double> sm(n), sv(n);
  double hl = 0.0, sums[4], gth[SS_NTHETA];
  const SSGradOut go{grad_r, grad_w, sums, gth};
  if (int rc = ss_core(x, n, lts, 1, w, r, chunk, &hl, nullptr, nullptr, sm.p, sv.p, false, &go)) return rc;
  launch_vec_lin(grad_r, grad_r, -2.0, n, grad_r, st0);      // ss_core left alpha there: d lml / d r = -alpha
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(lml, &hl, sizeof(double), hipMemcpyHostToDevice, st0));
  HIPCHK(hipMemcpyAsync(grad_theta, gth, (size_t)ntheta * sizeof(double), hipMemcpyHostToDevice, st0));
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

int lmm_dev_statespace_grad(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, int chunk, double* lml,
                            double* grad_r, double* grad_w, double* grad_theta) {
  return ss_dev_grad(x, n, gp, w, r, chunk, lml, grad_r, grad_w, grad_theta, 2);
}

int lmm_dev_statespace_grad_sho(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, int chunk, double* lml,
                                double* grad_r, double* grad_w, double* grad_theta) {
  return ss_dev_grad(x, n, gp, w, r, chunk, lml, grad_r, grad_w, grad_theta, 3);
}

// The same for a sum latent: grad_theta holds 6 values, the seeds of its first term in the library's order of the terms (Matern12,
// Matern32, SHO, Matern52), then those of its second: d lml / d V_c, d lml / d E_c and, SHO, d lml / d quality, with V_c = v0 v_c and
// E_c = s0 l_c the term's own variance and lengthscale (period); the slots behind the last seed are 0.
int lmm_dev_statespace_grad_sum(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, int chunk, double* lml,
                                double* grad_r, double* grad_w, double* grad_theta) {
  return ss_dev_grad(x, n, gp, w, r, chunk, lml, grad_r, grad_w, grad_theta, SS_NTHETA);
}

// Building block for tests beside lmm_dev_statespace_grad: grad_x (n values, device) = d lml / d x_t of ONE latent, Matern or SHO (the
// tag carries an SHO latent's quality, as in lmm_dev_statespace_grad_sho); exactly 0 where w = +Inf.
int lmm_dev_statespace_grad_x(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, int chunk, double* grad_x) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  std::shared_ptr<LatentSet> ls;
  if (int rc = ss_dev_prepare(!x || !gp || !w || !r || !grad_x || n <= 0 || chunk < 0, x, n, gp, ls, 1, true)) return rc;
  const Latent* lts = ls->lat.data();
  hipStream_t st0 = g.streams[0];
  Buf<double> sm(n), sv(n), al(n), gw(n), gd(n);
  double hl = 0.0, sums[4], gth[SS_NTHETA];
  const SSGradOut go{al.p, gw.p, sums, gth, gd.p};
  if (int rc = ss_core(x, n, lts, 1, w, r, chunk, &hl, nullptr, nullptr, sm.p, sv.p, false, &go)) return rc;
  launch_ss_grad_x(gd.p, w, n, 1, grad_x, st0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

// ---- the posterior object (DESIGN.md 4.18 "Posterior object") --------------------------------------------------------------------
// One O(n) conditioning pass keeps, per latent of the shard, the filtered and the full smoothed states; a query at new inputs is then
// one thread per (query, latent) (ss_interp_kernel) and the mixing of lmm_oilmm_mean_and_var_statespace.
struct lmm_ss_post {
  int n = 0, p = 0, m = 0, l0 = 0, l1 = 0;
  double sigma2 = 0.0;
  std::shared_ptr<LatentSet> ls;      // all m latents as the handle was built with them
  Buf<double> x;                      // the sorted inputs: n of cap
  Buf<double> fstate;                 // per latent of the shard, one after the other: cap x ss_state_comps(D_l), point-major, n rows filled
  Buf<double> H;                      // p x (l1 - l0), column-major: H = U sqrt(S) of the shard
  std::vector<size_t> off;            // latent l0 + k's offset into fstate / sstate: the blocks are strided by cap
  // Appending (DESIGN.md 4.18 "Appending observations"): rows beyond n are room for later points; the smoothed states are current for
  // the first smoothed_n points only (== n on a fresh handle) and are rebuilt from the filtered ones, without the data, when a query
  // in front of the last input needs them -- which a query entry point does through its const handle, hence `mutable`.
  int cap = 0;
  mutable int smoothed_n = 0;
  mutable Buf<double> sstate;         // laid out as fstate
  std::vector<double> U, S;           // host copies of the mixing matrix's factors (p x m, m): the front end projects new data with them
  double xlast = 0.0;                 // x[n - 1]
  double logpdf = 0.0;                // log p(all data so far), regulariser included
};

// latent k's offset into a state buffer whose blocks hold `cap` points
static std::vector<size_t> ss_post_offsets(const Latent* lts, int ms, int cap) {
  std::vector<size_t> off;
  size_t total = 0;
  for (int k = 0; k < ms; ++k) {
    off.push_back(total);
    total += (size_t)ss_state_comps(ss_latent_dim(lts[k])) * cap;
  }
  off.push_back(total);               // one behind the last: the buffer's size
  return off;
}

// The stored states of ms latents over n sorted inputs, as every reader takes them (device pointers but off): latent k's filtered and
// smoothed states lie off[k] doubles into fstate / sstate, in a block with room for cap >= n points, [point][component] or transposed.
enum SSLayout { SS_POINT_MAJOR, SS_COMPONENT_MAJOR };
struct SSStored { const double* x; int n, cap; const Latent* lts; int ms; const double* fstate; const double* sstate; const size_t* off; SSLayout layout; };
static SSStored ss_stored(const lmm_ss_post* P) {
  return {P->x.p, P->n, P->cap, P->ls->lat.data() + P->l0, P->l1 - P->l0, P->fstate.p, P->sstate.p, P->off.data(), SS_POINT_MAJOR};
}
static const size_t kNoOffset = 0;       // one latent's own buffers, as the lmm_dev_statespace_* building blocks are handed them
static SSStored ss_stored(const double* x, int n, const Latent* lt, const double* fstate, const double* sstate, SSLayout layout = SS_POINT_MAJOR) {
  return {x, n, n, lt, 1, fstate, sstate, &kNoOffset, layout};
}

// The zero-mean (add_mean: plus the latent's mean) marginals of the stored latents at the ns queries xsd: ml, vl [latent][ns] on the
// device (vl may be nullptr); SS_INTERP_DX: their derivatives with respect to the query instead (both given; launch_ss_interp_dx).
// Launches group consecutive latents of one model, LMM_MAX_BATCH at the most.  Queues on streams[0] and does not wait.
enum SSInterpWhat { SS_INTERP_MARGINALS, SS_INTERP_DX };
static void ss_interp_latents(const SSStored& S, const double* xsd, int ns, SSInterpWhat what, bool add_mean, double* ml, double* vl) {
  hipStream_t st0 = g.streams[0];
  const bool point_major = S.layout == SS_POINT_MAJOR, dx = what == SS_INTERP_DX;
  const auto no_buffers = [](int, int, int) { return size_t(1); };       // a launch allocates nothing: LMM_MAX_BATCH alone limits it
  ss_for_launches(S.ms, 0, [&](long long k) -> const Latent& { return S.lts[k]; }, no_buffers, [&](long long e0, int nb, int model, int D) {
    const int k0 = (int)e0;
    SSInterpArgs a{};
    a.x = S.x; a.n = S.n; a.xs = xsd; a.ns = ns;
    a.fstate = S.fstate + S.off[k0]; a.sstate = S.sstate + S.off[k0];
    a.state_stride = (size_t)ss_state_comps(D) * S.cap;
    a.comp_stride = point_major ? 1 : (size_t)S.n; a.point_stride = point_major ? (size_t)ss_state_comps(D) : 1;
    (dx ? a.dmean : a.mean) = ml + (size_t)k0 * ns; (dx ? a.dvar : a.var) = vl ? vl + (size_t)k0 * ns : nullptr;
    for (int j = 0; j < nb; ++j) ss_fill_lat(a.lat[j], S.lts[k0 + j], add_mean);
    (dx ? launch_ss_interp_dx : launch_ss_interp)(a, model, nb, st0);
  });
  HIPCHK(hipGetLastError());
}

int lmm_oilmm_statespace_posterior_create(const double* x, int n, const double* y, int p, const double* U, const double* S, int m,
                                          double sigma2, const lmm_gp_t* gps, int latent_begin, int latent_end, lmm_ss_post_t** out,
                                          double* out_logpdf) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  SSTrain T;
  if (int rc = ss_train(!y || !out, x, n, y, p, U, S, m, sigma2, gps, latent_begin, latent_end, T, false, [&] { *out = nullptr; return 0; })) return rc;
  hipStream_t st0 = g.streams[0];
  const auto& [ls, lts, xd, yd, l0, l1, ms, mk, Fr] = T;
  std::unique_ptr<lmm_ss_post> P(new lmm_ss_post());      // a throw below (a failed allocation) frees what it holds
  P->n = n; P->p = p; P->m = m; P->l0 = l0; P->l1 = l1; P->sigma2 = sigma2; P->ls = ls;
  P->cap = n; P->smoothed_n = n;
  P->U.assign(U, U + (size_t)p * m); P->S.assign(S, S + m);
  std::vector<SSEntry> es(ms);
  for (int k = 0; k < ms; ++k) es[k] = SSEntry{lts + l0 + k, Fr.w.p + (size_t)k * n, Fr.r.p + (size_t)k * n};
  P->off = ss_post_offsets(lts + l0, ms, n);
  const size_t total = P->off[ms];
  P->x = Buf<double>((size_t)n);
  P->fstate = Buf<double>(std::max<size_t>(total, 1)); P->sstate = Buf<double>(std::max<size_t>(total, 1));
  HIPCHK(hipMemcpyAsync(P->x.p, xd.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st0));
  const std::vector<double> Hs = shard_H(U, S, p, l0, ms);
  P->H = Buf<double>(Hs.size());
  HIPCHK(hipMemcpyAsync(P->H.p, Hs.data(), Hs.size() * sizeof(double), hipMemcpyHostToDevice, st0));
  std::vector<double> lml(mk, 0.0);
  const SSKeep keep{P->fstate.p, P->sstate.p};
  if (int rc = ss_core_entries(P->x.p, n, es.data(), ms, 0, lml.data(), nullptr, nullptr, nullptr, nullptr, false, nullptr, &keep)) return rc;
  HIPCHK(hipStreamSynchronize(st0));
  double value = 0.0;                       // the sum of lmm_oilmm_logpdf_statespace, in its order
  for (int k = 0; k < ms; ++k) value += lml[k];
  value += Fr.reg;
  if (out_logpdf) *out_logpdf = value;
  P->logpdf = value;
  HIPCHK(hipMemcpy(&P->xlast, P->x.p + (n - 1), sizeof(double), hipMemcpyDeviceToHost));
  *out = P.release();
  return LMM_OK;
  LMM_CATCH
}

int lmm_statespace_post_destroy(lmm_ss_post_t* post) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (post) {
    if (g.init) (void)hipDeviceSynchronize();
    delete post;
  }
  return LMM_OK;
}

// ---- appending observations (DESIGN.md 4.18 "Appending observations") ------------------------------------------------------------
// The RTS pass over all n kept filtered states (launch_ss_smooth_kept): O(n), without the data.  Returns with streams[0] drained.
static int ss_post_smooth(const lmm_ss_post* P) {
  if (P->smoothed_n == P->n) return LMM_OK;
  hipStream_t st0 = g.streams[0];
  const int n = P->n, ms = P->l1 - P->l0;
  const Latent* lts = P->ls->lat.data() + P->l0;
  const SSChunks plan = ss_plan_chunks(n, 0);
  const auto bytes = [&](int, int D, int nch) { return ss_bwd_agg_elems(D, nch) * sizeof(double); };
  ss_for_launches(ms, plan.nch, [&](long long k) -> const Latent& { return lts[k]; }, bytes, [&](long long e0, int nb, int model, int D) {
    const int k0 = (int)e0;
    Buf<double> bagg((size_t)nb * ss_bwd_agg_elems(D, plan.nch));
    SSArgs a{};
    a.x = P->x.p; a.n = n; a.chunk = plan.chunk; a.nch = plan.nch;
    a.bagg = bagg.p;
    a.fkeep = P->fstate.p + P->off[k0]; a.sstate = P->sstate.p + P->off[k0];
    a.state_stride = (size_t)ss_state_comps(D) * P->cap;
    for (int j = 0; j < nb; ++j) ss_fill_lat(a.lat[j], lts[k0 + j], false);
    launch_ss_smooth_kept(a, model, nb, st0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st0));          // bagg goes back to the pool
  });
  P->smoothed_n = n;
  return LMM_OK;
}

// What a query entry point does with a handle whose smoothed states are behind: a query reads one only when it lies in front of the
// last input (ss_interp's has_next), so one small kernel and a 4-byte download decide (ss_first_flagged's pattern) and a batch of pure
// forecasts -- a query equal to the last input is one -- never pays the O(n) pass.
static int ss_post_ensure_smoothed(const lmm_ss_post* P, const double* xsd, int ns) {
  if (P->smoothed_n == P->n) return LMM_OK;
  hipStream_t st0 = g.streams[0];
  Buf<int> flag(1);
  int h = 0;
  launch_ss_any_below(xsd, ns, P->xlast, flag.p, st0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&h, flag.p, sizeof(int), hipMemcpyDeviceToHost, st0));
  HIPCHK(hipStreamSynchronize(st0));
  return h ? ss_post_smooth(P) : (int)LMM_OK;
}

// Room for n_total points: new buffers, one device-to-device copy of the n filled rows of every block, then the handle takes them (a
// failed allocation throws before the handle is touched).  The smoothed states are copied too: they stay current for smoothed_n points.
static void ss_post_grow(lmm_ss_post* P, int n_total) {
  if (n_total <= P->cap) return;
  hipStream_t st0 = g.streams[0];
  const int ms = P->l1 - P->l0, n = P->n;
  const Latent* lts = P->ls->lat.data() + P->l0;
  const std::vector<size_t> off = ss_post_offsets(lts, ms, n_total);
  Buf<double> x((size_t)n_total), fs(std::max<size_t>(off[ms], 1)), ss(std::max<size_t>(off[ms], 1));
  HIPCHK(hipMemcpyAsync(x.p, P->x.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st0));
  for (int k = 0; k < ms; ++k) {
    const size_t bytes = (size_t)ss_state_comps(ss_latent_dim(lts[k])) * n * sizeof(double);
    HIPCHK(hipMemcpyAsync(fs.p + off[k], P->fstate.p + P->off[k], bytes, hipMemcpyDeviceToDevice, st0));
    HIPCHK(hipMemcpyAsync(ss.p + off[k], P->sstate.p + P->off[k], bytes, hipMemcpyDeviceToDevice, st0));
  }
  HIPCHK(hipStreamSynchronize(st0));            // the old buffers go back to the pool below
  P->x = std::move(x); P->fstate = std::move(fs); P->sstate = std::move(ss);
  P->off = off; P->cap = n_total;
}

// The launch loop of a scored scan, a filter over `items` points per latent that ends in lml[k] (host, ms values): from a stored state
// (SSFromArgs) or over a window's backward chain (SSLpdfArgs).  It holds the plan, the launch groups within the byte budget and their
// buffers (none with one chunk: the single launch); a0 is the launch's arguments but chunk, nch, agg, part and lat, and fill(a, k0, nb)
// sets what belongs to the latents [k0, k0 + nb) of a launch.  Returns with streams[0] drained.
template <typename Args, typename Fill>
static void ss_scored_scan(const Latent* lts, int ms, int items, int chunk, const Args& a0,
                           void (*launch)(const Args&, int, int, double*, hipStream_t), double* lml, Fill&& fill) {
  hipStream_t st0 = g.streams[0];
  const SSChunks plan = ss_plan_chunks(items, chunk);
  const auto bytes = [&](int, int D, int nch) { return (ss_fwd_agg_elems(D, nch) + (size_t)nch) * sizeof(double); };
  ss_for_launches(ms, plan.nch, [&](long long j) -> const Latent& { return lts[j]; }, bytes, [&](long long e0, int nb, int model, int D) {
    const int k0 = (int)e0, nch = plan.nch;
    Buf<double> agg, part, lmld(nb);
    if (nch > 1) { agg = Buf<double>((size_t)nb * ss_fwd_agg_elems(D, nch)); part = Buf<double>((size_t)nb * nch); }
    Args a = a0;
    a.chunk = plan.chunk; a.nch = nch; a.agg = agg.p; a.part = part.p;
    fill(a, k0, nb);
    launch(a, model, nb, lmld.p, st0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(lml + k0, lmld.p, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, st0));
    HIPCHK(hipStreamSynchronize(st0));          // the buffers above go back to the pool
  });
}

// The filter over k new points from a stored state, per launch group of the ms latents: latent j reads init[j] (device, packed) at
// input x0 and writes its k states to out[j] (device, point-major); w, r: [latent][k] on the device; lml: ms host values.
static void ss_filter_from(const double* xd, int k, double x0, const Latent* lts, int ms, const double* w, const double* r, int chunk,
                           const double* const* init, double* const* out, double* fmean, double* fvar, double* lml) {
  SSFromArgs a0{};
  a0.x = xd; a0.n = k; a0.x0 = x0;
  ss_scored_scan(lts, ms, k, chunk, a0, launch_ss_filter_from, lml, [&](SSFromArgs& a, int k0, int nb) {
    a.fmean = fmean ? fmean + (size_t)k0 * k : nullptr; a.fvar = fvar ? fvar + (size_t)k0 * k : nullptr;
    for (int j = 0; j < nb; ++j) {
      const Latent& L = lts[k0 + j];
      ss_fill_kernel(a.lat[j], L);
      a.lat[j].w = w + (size_t)(k0 + j) * k; a.lat[j].r = r + (size_t)(k0 + j) * k;
      a.lat[j].init = init[k0 + j]; a.lat[j].out = out[k0 + j];
    }
  });
}

int lmm_oilmm_statespace_post_append(lmm_ss_post_t* post, const double* x_new, int k, const double* y_new, double* out_increment) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!post || k < 0) return fail(LMM_ERR_ARG, "bad arguments");
  if (g_f32) return ss_refuse_f32();
  if (k == 0) {
    if (out_increment) *out_increment = 0.0;
    return LMM_OK;
  }
  if (!x_new || !y_new) return fail(LMM_ERR_ARG, "bad arguments");
  lmm_ss_post* P = post;
  const int n = P->n, p = P->p, m = P->m, ms = P->l1 - P->l0;
  if ((long long)n + k > INT_MAX) return fail(LMM_ERR_ARG, "state-space posterior: %d points and %d more are too many", n, k);
  hipStream_t st0 = g.streams[0];
  const Latent* lts = P->ls->lat.data();
  DevIn xd(x_new, (size_t)k, st0), yd(y_new, (size_t)k * p, st0);
  // every refusal comes before the handle is touched
  if (ss_first_flagged(launch_ss_finite, xd.p, k) != INT_MAX)
    return fail(LMM_ERR_ARG, "state-space posterior: x_new[%d] is not finite", g.err_info);
  if (int rc = ss_check_sorted(xd.p, k)) return rc;
  double ends[2];
  HIPCHK(hipMemcpyAsync(&ends[0], xd.p, sizeof(double), hipMemcpyDeviceToHost, st0));
  HIPCHK(hipMemcpyAsync(&ends[1], xd.p + (k - 1), sizeof(double), hipMemcpyDeviceToHost, st0));
  HIPCHK(hipStreamSynchronize(st0));
  if (ends[0] < P->xlast) {
    g.err_latent = -1; g.err_info = 0;
    return fail(LMM_ERR_ARG, "state-space posterior: appended points lie at or behind the last input (x_new[0] = %g is in front of %g)",
                ends[0], P->xlast);
  }
  SSFront Fr;
  if (int rc = ss_front(yd.p, k, p, P->U.data(), P->S.data(), m, P->sigma2, lts, P->l0, P->l1, Fr, false, n)) return rc;
  if (n + k > P->cap) ss_post_grow(P, (int)std::min<long long>(INT_MAX, std::max<long long>(2ll * P->cap, (long long)n + k)));      // geometric
  HIPCHK(hipMemcpyAsync(P->x.p + n, xd.p, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, st0));
  std::vector<const double*> init(ms);
  std::vector<double*> outp(ms);
  for (int j = 0; j < ms; ++j) {
    const size_t comps = (size_t)ss_state_comps(ss_latent_dim(lts[P->l0 + j]));
    init[j] = P->fstate.p + P->off[j] + (size_t)(n - 1) * comps;
    outp[j] = P->fstate.p + P->off[j] + (size_t)n * comps;
  }
  std::vector<double> lml(std::max(ms, 1), 0.0);
  ss_filter_from(P->x.p + n, k, P->xlast, lts + P->l0, ms, Fr.w.p, Fr.r.p, 0, init.data(), outp.data(), nullptr, nullptr, lml.data());
  HIPCHK(hipStreamSynchronize(st0));
  double inc = 0.0;
  for (int j = 0; j < ms; ++j) inc += lml[j];
  inc += Fr.reg;
  P->n = n + k; P->xlast = ends[1]; P->logpdf += inc;       // smoothed_n stays: the smoothed states are now behind
  if (out_increment) *out_increment = inc;
  return LMM_OK;
  LMM_CATCH
}

int lmm_statespace_post_smooth(lmm_ss_post_t* post) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!post) return fail(LMM_ERR_ARG, "bad arguments");
  if (g_f32) return ss_refuse_f32();
  return ss_post_smooth(post);
  LMM_CATCH
}

int lmm_statespace_post_reserve(lmm_ss_post_t* post, int n_total) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!post) return fail(LMM_ERR_ARG, "bad arguments");
  ss_post_grow(post, n_total);
  return LMM_OK;
  LMM_CATCH
}

int lmm_statespace_post_size(const lmm_ss_post_t* post, int* n, int* smoothed_n, int* cap) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!post) return fail(LMM_ERR_ARG, "bad arguments");
  if (n) *n = post->n;
  if (smoothed_n) *smoothed_n = post->smoothed_n;
  if (cap) *cap = post->cap;
  return LMM_OK;
}

// Building block for tests beside lmm_dev_statespace_filter: the filter of ONE latent over k points from the packed state `state0`
// (device) at input x0 <= x[0].  fstate: k x ss_state_comps(D), point-major.
int lmm_dev_statespace_filter_from(const double* state0, double x0, const double* x, int k, const lmm_gp_t* gp, const double* w,
                                   const double* r, int chunk, double* fmean, double* fvar, double* fstate, double* lml) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  std::shared_ptr<LatentSet> ls;
  const bool bad = !state0 || !x || !gp || !w || !r || !fmean || !fvar || !fstate || !lml || k <= 0 || chunk < 0 || !std::isfinite(x0);
  if (int rc = ss_dev_prepare(bad, x, k, gp, ls)) return rc;
  hipStream_t st0 = g.streams[0];
  double first = 0.0;
  HIPCHK(hipMemcpy(&first, x, sizeof(double), hipMemcpyDeviceToHost));
  if (!(first >= x0)) return fail(LMM_ERR_ARG, "state-space filter: x[0] = %g lies in front of the given state's input x0 = %g", first, x0);
  double h = 0.0;
  ss_filter_from(x, k, x0, ls->lat.data(), 1, w, r, chunk, &state0, &fstate, fmean, fvar, &h);
  HIPCHK(hipMemcpyAsync(lml, &h, sizeof(double), hipMemcpyHostToDevice, st0));
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

int lmm_oilmm_statespace_post_mean_and_var(const lmm_ss_post_t* post, const double* xs, int ns, int add_noise, double* mean_out,
                                           double* var_out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!post || !xs || !mean_out || ns < 1) return fail(LMM_ERR_ARG, "bad arguments");
  if (g_f32) return ss_refuse_f32();
  const lmm_ss_post* P = post;
  const int p = P->p, ms = P->l1 - P->l0;
  hipStream_t st0 = g.streams[0];
  DevIn xsd(xs, (size_t)ns, st0);
  if (int rc = ss_check_finite(xsd.p, ns)) return rc;
  if (int rc = ss_post_ensure_smoothed(P, xsd.p, ns)) return rc;
  Buf<double> ml((size_t)ns * std::max(ms, 1)), vl((size_t)ns * std::max(ms, 1));
  ss_interp_latents(ss_stored(P), xsd.p, ns, SS_INTERP_MARGINALS, true, ml.p, var_out ? vl.p : nullptr);
  DevOut mo(mean_out, (size_t)ns * p), vo(var_out, (size_t)ns * p);
  mix_marginals(ml.p, ns, ms, P->H.p, p, 1, 0.0, 0.0, mo.p, st0);
  if (var_out) mix_marginals(vl.p, ns, ms, P->H.p, p, 2, kDefaultJit.default_jitter, add_noise ? P->sigma2 : 0.0, vo.p, st0);
  mo.finish(st0); vo.finish(st0);
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

// The pullback of lmm_oilmm_statespace_post_mean_and_var to the queries: per (query, latent) the derivatives of the latent's mean and
// variance (ss_interp_dx_kernel), contracted with H and the cotangents in latent order (launch_ss_contract_dx).  The added sigma2 does
// not depend on xs.
int lmm_oilmm_statespace_post_mean_and_var_grad_xs(const lmm_ss_post_t* post, const double* xs, int ns, const double* dmean,
                                                   const double* dvar, double* grad_xs) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!post || !xs || !grad_xs || ns < 1) return fail(LMM_ERR_ARG, "bad arguments");
  if (!dmean && !dvar) return fail(LMM_ERR_ARG, "state-space posterior: dmean and dvar are both NULL (one cotangent is needed)");
  if (g_f32) return ss_refuse_f32();
  const lmm_ss_post* P = post;
  if (int rc = ss_check_latents(P->ls->lat.data(), P->m, true)) return rc;       // component 2 of a sum latent's state is not f'
  const int p = P->p, ms = P->l1 - P->l0;
  hipStream_t st0 = g.streams[0];
  DevIn xsd(xs, (size_t)ns, st0);
  if (int rc = ss_check_finite(xsd.p, ns)) return rc;
  if (int rc = ss_post_ensure_smoothed(P, xsd.p, ns)) return rc;
  DevIn dm(dmean, (size_t)ns * p, st0), dv(dvar, (size_t)ns * p, st0);
  Buf<double> ml((size_t)ns * std::max(ms, 1)), vl((size_t)ns * std::max(ms, 1));
  ss_interp_latents(ss_stored(P), xsd.p, ns, SS_INTERP_DX, false, ml.p, vl.p);
  DevOut go(grad_xs, (size_t)ns);
  launch_ss_contract_dx(dm.p, dv.p, P->H.p, p, ms, ml.p, vl.p, ns, go.p, st0);
  HIPCHK(hipGetLastError());
  go.finish(st0);
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

// Building blocks for tests beside lmm_dev_statespace_smooth (DEVICE pointers, one latent, gp on the host, its mean not read).
int lmm_dev_statespace_states(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, int chunk, double* fstate,
                              double* sstate) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  std::shared_ptr<LatentSet> ls;
  if (int rc = ss_dev_prepare(!x || !gp || !w || !r || !fstate || !sstate || n <= 0 || chunk < 0, x, n, gp, ls)) return rc;
  const Latent* lts = ls->lat.data();
  const SSEntry e{lts, w, r};
  const SSKeep keep{fstate, sstate};
  return ss_core_entries(x, n, &e, 1, chunk, nullptr, nullptr, nullptr, nullptr, nullptr, false, nullptr, &keep);
  LMM_CATCH
}

// point_major = 0: the states are comps x n (what the filter writes for itself) instead of the n x comps the library keeps; the layout
// experiment of DESIGN.md 4.18 "Posterior object" (tools/statespace_posterior_bench.py)
int lmm_dev_statespace_interp_layout(const double* x, int n, const lmm_gp_t* gp, const double* fstate, const double* sstate,
                                     int point_major, const double* xs, int ns, double* mean, double* var) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  std::shared_ptr<LatentSet> ls;
  const bool bad = !x || !gp || !fstate || !sstate || !xs || !mean || !var || n <= 0 || ns < 1;
  if (int rc = ss_dev_prepare(bad, x, n, gp, ls)) return rc;
  const Latent* lts = ls->lat.data();
  if (int rc = ss_check_finite(xs, ns)) return rc;
  const SSLayout layout = point_major ? SS_POINT_MAJOR : SS_COMPONENT_MAJOR;
  ss_interp_latents(ss_stored(x, n, lts, fstate, sstate, layout), xs, ns, SS_INTERP_MARGINALS, false, mean, var);
  HIPCHK(hipStreamSynchronize(g.streams[0]));
  return LMM_OK;
  LMM_CATCH
}

int lmm_dev_statespace_interp(const double* x, int n, const lmm_gp_t* gp, const double* fstate, const double* sstate, const double* xs,
                              int ns, double* mean, double* var) {
  return lmm_dev_statespace_interp_layout(x, n, gp, fstate, sstate, 1, xs, ns, mean, var);
}

// ---- sampling (DESIGN.md 4.18 "Sampling") ----------------------------------------------------------------------------------------
// The affine-scan launches of the (latent, sample) pairs of the ms latents lts[0 .. ms) and N samples, `rows` points per pair: pair e
// is (latent e / N, sample e % N), and the pairs run in launches of one model.  a: the launch's arguments but chunk, nch, agg and lat;
// fill(lat, k, q, zoff) sets the pointers of pair (k, q), whose normals lie zoff doubles into a sample's (the latents one after the
// other, D_l rows values each).  Returns with streams[0] drained.
template <typename Args, typename Fill>
static void ss_pair_launches(const Latent* lts, int ms, int N, int rows, int chunk, bool add_mean, const Args& a0,
                             void (*launch)(const Args&, int, int, hipStream_t), Fill&& fill) {
  hipStream_t st0 = g.streams[0];
  const SSChunks plan = ss_plan_chunks(rows, chunk);
  std::vector<size_t> zoff(std::max(ms, 1), 0);
  for (int k = 1; k < ms; ++k) zoff[k] = zoff[k - 1] + (size_t)ss_latent_dim(lts[k - 1]) * rows;
  const auto bytes = [](int, int D, int nch) { return ss_aff_agg_elems(D, nch) * sizeof(double); };
  ss_for_launches((long long)ms * N, plan.nch, [&](long long e) -> const Latent& { return lts[e / N]; }, bytes,
                  [&](long long e0, int nb, int model, int D) {
    Buf<double> agg((size_t)nb * ss_aff_agg_elems(D, plan.nch));
    Args a = a0;
    a.chunk = plan.chunk; a.nch = plan.nch; a.agg = agg.p;
    for (int j = 0; j < nb; ++j) {
      const int k = (int)((e0 + j) / N), q = (int)((e0 + j) % N);
      ss_fill_lat(a.lat[j], lts[k], add_mean);
      fill(a.lat[j], k, q, zoff[k]);
    }
    launch(a, model, nb, st0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st0));          // agg goes back to the pool
  });
}

// Prior paths of the ms latents lts[0 .. ms) for N samples: f[sample][latent][n] on the device, with the latent's mean when add_mean.
// z: sample 0's normals of lts[0] on the device, the latents one after the other (D_l n values each, component-major), the samples
// z_stride doubles apart.  Returns with streams[0] drained.
static int ss_paths(const double* xd, int n, const Latent* lts, int ms, int N, const double* z, size_t z_stride, int chunk, bool add_mean,
                    double* f) {
  SSPathArgs a{};
  a.x = xd; a.n = n;
  ss_pair_launches(lts, ms, N, n, chunk, add_mean, a, launch_ss_path, [&](SSPathLat& o, int k, int q, size_t zoff) {
    o.z = z + (size_t)q * z_stride + zoff; o.f = f + ((size_t)q * ms + k) * n;
  });
  return LMM_OK;
}

// Pathwise conditioning (Matheron's rule): the zero-mean prior paths f[sample][latent][n] become posterior paths given the latents'
// data r with noise w ([latent][n]; w = +Inf: unobserved): f += the smoothed mean of r - f - sqrt(w) xi (+ the latent's mean when
// add_mean).  xi: sample 0's normals of lts[0], n per latent, the samples xi_stride doubles apart.  The samples are further entries of
// the latent dimension of the filter and smoother, [latent][sample], with the latent's w and their own data.
static int ss_condition(const double* xd, int n, const Latent* lts, int ms, int N, const double* w, const double* r, const double* xi,
                        size_t xi_stride, int chunk, bool add_mean, double* f) {
  if (ms == 0) return LMM_OK;
  hipStream_t st0 = g.streams[0];
  const size_t ne = (size_t)ms * N;
  Buf<double> rp(ne * n), sm(ne * n);
  launch_ss_pathwise(r, w, f, xi, xi_stride, n, ms, N, rp.p, st0);
  HIPCHK(hipGetLastError());
  std::vector<SSEntry> es(ne);
  for (size_t e = 0; e < ne; ++e) es[e] = SSEntry{lts + e / N, w + (e / N) * n, rp.p + e * n};
  if (int rc = ss_core_entries(xd, n, es.data(), (int)ne, chunk, nullptr, nullptr, nullptr, sm.p, nullptr, add_mean)) return rc;
  launch_ss_addpath(f, sm.p, n, ms, N, st0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st0));            // rp and sm go back to the pool
  return LMM_OK;
}

// samples of one group: the buffers of a group stay within LMM_SS_BATCH_BYTES, and a group is one grid dimension of the elementwise kernels
static int ss_sample_group(int n, int ms, int N) {
  const size_t per = (size_t)std::max(ms, 1) * n * sizeof(double) * 4;
  return (int)std::max<size_t>(1, std::min<size_t>(std::min(N, 32768), LMM_SS_BATCH_BYTES / per));
}

// The normals of samples [q0, q0 + ng) of one shard on the device: src holds `per_sample` doubles per sample, of which the shard reads
// `count` from `offset` on.  A device pointer is used where it lies; a host pointer's slices are uploaded side by side.
struct SSNormals {
  const double* p = nullptr; size_t stride = 0;
  Buf<double> own;
  SSNormals(const double* src, size_t per_sample, size_t offset, size_t count, int q0, int ng, hipStream_t st) {
    if (src == nullptr) return;
    if (is_device_ptr(src)) { p = src + (size_t)q0 * per_sample + offset; stride = per_sample; return; }
    own = Buf<double>(std::max<size_t>(count, 1) * ng);
    for (int q = 0; q < ng && count > 0; ++q)
      HIPCHK(hipMemcpyAsync(own.p + (size_t)q * count, src + (size_t)(q0 + q) * per_sample + offset, count * sizeof(double),
                            hipMemcpyHostToDevice, st));
    p = own.p; stride = count;
  }
};

// body(q0, ng) for the samples [q0, q0 + ng) of every group (ss_sample_group over `rows` points per sample and latent)
template <typename Body>
static int ss_for_sample_groups(int rows, int ms, int nsamples, Body&& body) {
  const int group = ss_sample_group(rows, ms, nsamples);
  for (int q0 = 0; q0 < nsamples; q0 += group)
    if (int rc = body(q0, std::min(group, nsamples - q0))) return rc;
  return LMM_OK;
}

// The sampling entry points' loop: per group, paths(q0, ng, f) leaves the latent paths of samples [q0, q0 + ng) in f[sample][latent
// of the shard][rows] on the device, and the mixing of lmm_lmm_rand (reference src/oilmm.jl:50-53), H f + sqrt(sigma2) eps, writes
// rows x p per sample to od (device).  eps: host or device, rows x p per sample (nullptr: no noise); Hd: p x ms on the device.
template <typename Paths>
static int ss_sample_mix(int rows, int group_rows, int ms, int p, const double* Hd, double sigma2, const double* eps, int nsamples,
                         double* od, Paths&& paths) {
  hipStream_t st0 = g.streams[0];
  return ss_for_sample_groups(group_rows, ms, nsamples, [&](int q0, int ng) {
    SSNormals epsd(eps, (size_t)rows * p, 0, (size_t)rows * p, q0, ng, st0);
    Buf<double> f((size_t)ng * std::max(ms, 1) * rows);
    if (int rc = paths(q0, ng, f.p)) return rc;
    for (int q = 0; q < ng; ++q)
      launch_mix(f.p + (size_t)q * ms * rows, rows, ms, Hd, p, 1, 0.0, 0.0, eps ? epsd.p + (size_t)q * epsd.stride : nullptr,
                 std::sqrt(sigma2), od + (size_t)(q0 + q) * rows * p, st0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st0));            // the group's buffers go back to the pool
    return (int)LMM_OK;
  });
}

int lmm_oilmm_rand_statespace(const double* x, int n, const double* y, int p, const double* U, const double* S, int m, double sigma2,
                              const lmm_gp_t* gps, int latent_begin, int latent_end, int add_noise, int nsamples, const double* z,
                              const double* xi, const double* eps, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  SSTrain T;
  const int rc0 = ss_train(!out, x, n, y, p, U, S, m, sigma2, gps, latent_begin, latent_end, T, false, [&] {      // y may be NULL: the prior
    if (nsamples < 1) return fail(LMM_ERR_ARG, "nsamples must be >= 1 (nsamples = %d)", nsamples);
    if (!z) return fail(LMM_ERR_ARG, "z is NULL");
    if (y && !xi) return fail(LMM_ERR_ARG, "xi is NULL (a posterior sample needs it)");
    return add_noise && !eps ? fail(LMM_ERR_ARG, "eps is NULL") : (int)LMM_OK;
  });
  if (rc0) return rc0;
  hipStream_t st0 = g.streams[0];
  const Latent* lts = T.lts;
  const int l0 = T.l0, l1 = T.l1, ms = T.ms;
  size_t zall = 0, zbefore = 0, zshard = 0;        // doubles of one sample's z: every latent, those before the shard, the shard's
  for (int l = 0; l < m; ++l) {
    const size_t c = (size_t)ss_latent_dim(lts[l]) * n;
    zall += c;
    if (l < l0) zbefore += c;
    else if (l < l1) zshard += c;
  }
  Uploaded Hd(shard_H(U, S, p, l0, ms), st0);
  DevOut od(out, (size_t)n * p * nsamples);
  const int rc = ss_sample_mix(n, n, ms, p, Hd.buf.p, sigma2, add_noise ? eps : nullptr, nsamples, od.p, [&](int q0, int ng, double* f) {
    SSNormals zd(z, zall, zbefore, zshard, q0, ng, st0), xid(y ? xi : nullptr, (size_t)m * n, (size_t)l0 * n, (size_t)ms * n, q0, ng, st0);
    if (int rc = ss_paths(T.xd.p, n, lts + l0, ms, ng, zd.p, zd.stride, 0, y == nullptr, f)) return rc;
    if (y == nullptr) return (int)LMM_OK;
    return ss_condition(T.xd.p, n, lts + l0, ms, ng, T.Fr.w.p, T.Fr.r.p, xid.p, xid.stride, 0, true, f);
  });
  if (rc) return rc;
  od.finish(st0);
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

// Building blocks for tests beside lmm_dev_statespace_smooth: ONE latent from DEVICE pointers, its mean not read.  f: [sample][n].
static int ss_dev_sample(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, const double* z, const double* xi,
                         int nsamples, int chunk, double* f) {
  std::shared_ptr<LatentSet> ls;
  if (int rc = ss_dev_prepare(n <= 0 || chunk < 0, x, n, gp, ls, nsamples)) return rc;
  const Latent* lts = ls->lat.data();
  const size_t zs = (size_t)ss_latent_dim(lts[0]) * n;
  return ss_for_sample_groups(n, 1, nsamples, [&](int q0, int ng) {
    double* fq = f + (size_t)q0 * n;
    if (int rc = ss_paths(x, n, lts, 1, ng, z + (size_t)q0 * zs, zs, chunk, false, fq)) return rc;
    if (w == nullptr) return (int)LMM_OK;
    return ss_condition(x, n, lts, 1, ng, w, r, xi + (size_t)q0 * n, (size_t)n, chunk, false, fq);
  });
}

int lmm_dev_statespace_sample(const double* x, int n, const lmm_gp_t* gp, const double* z, int nsamples, int chunk, double* f) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!x || !gp || !z || !f) return fail(LMM_ERR_ARG, "bad arguments");
  return ss_dev_sample(x, n, gp, nullptr, nullptr, z, nullptr, nsamples, chunk, f);
  LMM_CATCH
}

int lmm_dev_statespace_sample_posterior(const double* x, int n, const lmm_gp_t* gp, const double* w, const double* r, const double* z,
                                        const double* xi, int nsamples, int chunk, double* f) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!x || !gp || !w || !r || !z || !xi || !f) return fail(LMM_ERR_ARG, "bad arguments");
  return ss_dev_sample(x, n, gp, w, r, z, xi, nsamples, chunk, f);
  LMM_CATCH
}

// ---- sampling from the posterior object (DESIGN.md 4.18 "Sampling from the posterior object") ------------------------------------
// first = #{t : x_t <= lo}, count = #{t : x_t <= hi} - first; xsd != nullptr: (lo, hi) = (xsd[0], xsd[ns - 1]), read on the device
static void ss_window_bounds(const double* xd, int n, const double* xsd, int ns, double lo, double hi, int* first, int* count) {
  hipStream_t st0 = g.streams[0];
  Buf<int> ab(2);
  int h[2] = {0, 0};
  launch_ss_window_bounds(xd, n, xsd, ns, lo, hi, ab.p, st0);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h, ab.p, 2 * sizeof(int), hipMemcpyDeviceToHost, st0));
  HIPCHK(hipStreamSynchronize(st0));
  *first = h[0]; *count = h[1] - h[0];
}

// The window of the queries xsd (device, ns values): they must be finite and non-decreasing (LMM_ERR_ARG with the first offending
// index in the error detail's `info`).  src: W = ns + count entries (launch_ss_window).
struct SSWindow { int first = 0, count = 0, W = 0; Buf<int> src; };
static int ss_window(const double* xd, int n, const double* xsd, int ns, SSWindow& w) {
  if (int rc = ss_check_finite(xsd, ns)) return rc;
  if (int rc = ss_check_sorted(xsd, ns)) return rc;
  ss_window_bounds(xd, n, xsd, ns, 0.0, 0.0, &w.first, &w.count);
  if ((long long)ns + w.count > INT_MAX) return fail(LMM_ERR_ARG, "state-space posterior: the window of %d queries and %d points is too long", ns, w.count);
  w.W = ns + w.count;
  w.src = Buf<int>((size_t)w.W);
  launch_ss_window(xd, n, xsd, ns, w.first, w.count, w.src.p, g.streams[0]);
  HIPCHK(hipGetLastError());
  return LMM_OK;
}

// Posterior paths of the stored latents at the sorted queries for N samples: f[sample][latent][ns] on the device, with the latent's
// mean when add_mean.  z: sample 0's normals of S.lts[0] on the device, the latents one after the other (D_l W values each,
// component-major over window positions), the samples z_stride doubles apart.  Returns with streams[0] drained.
static int ss_post_paths(const SSStored& S, const double* xsd, int ns, const SSWindow& w, int N, const double* z, size_t z_stride, int chunk,
                         bool add_mean, double* f) {
  SSPostArgs a{};
  a.x = S.x; a.n = S.n; a.xs = xsd; a.ns = ns; a.src = w.src.p; a.first = w.first; a.W = w.W;
  ss_pair_launches(S.lts, S.ms, N, w.W, chunk, add_mean, a, launch_ss_post_path, [&](SSPostLat& o, int k, int q, size_t zoff) {
    o.fstate = S.fstate + S.off[k]; o.sstate = S.sstate + S.off[k]; o.z = z + (size_t)q * z_stride + zoff; o.f = f + ((size_t)q * S.ms + k) * ns;
  });
  return LMM_OK;
}

int lmm_statespace_post_window(const lmm_ss_post_t* post, double lo, double hi, int* first, int* count) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!post || !first || !count) return fail(LMM_ERR_ARG, "bad arguments");
  if (!std::isfinite(lo) || !std::isfinite(hi) || lo > hi)
    return fail(LMM_ERR_ARG, "state-space posterior: a window needs finite lo <= hi (lo = %g, hi = %g)", lo, hi);
  if (post->smoothed_n < post->n && lo < post->xlast)       // a sampler over this window reads a smoothed state
    if (int rc = ss_post_smooth(post)) return rc;
  ss_window_bounds(post->x.p, post->n, nullptr, 0, lo, hi, first, count);
  return LMM_OK;
  LMM_CATCH
}

int lmm_oilmm_statespace_post_rand(const lmm_ss_post_t* post, const double* xs, int ns, const double* z, const double* eps, int nsamples,
                                   int add_noise, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!post || !xs || !out || ns < 1) return fail(LMM_ERR_ARG, "bad arguments");
  if (g_f32) return ss_refuse_f32();
  if (nsamples < 1) return fail(LMM_ERR_ARG, "nsamples must be >= 1 (nsamples = %d)", nsamples);
  if (!z) return fail(LMM_ERR_ARG, "z is NULL");
  if (add_noise && !eps) return fail(LMM_ERR_ARG, "eps is NULL");
  const lmm_ss_post* P = post;
  const int p = P->p, ms = P->l1 - P->l0;
  const Latent* lts = P->ls->lat.data() + P->l0;
  hipStream_t st0 = g.streams[0];
  DevIn xsd(xs, (size_t)ns, st0);
  SSWindow w;
  if (int rc = ss_window(P->x.p, P->n, xsd.p, ns, w)) return rc;
  if (int rc = ss_post_ensure_smoothed(P, xsd.p, ns)) return rc;
  size_t zshard = 0;                               // doubles of one sample's z
  for (int k = 0; k < ms; ++k) zshard += (size_t)ss_latent_dim(lts[k]) * w.W;
  DevOut od(out, (size_t)ns * p * nsamples);
  const int rc = ss_sample_mix(ns, std::max(w.W, ns), ms, p, P->H.p, P->sigma2, add_noise ? eps : nullptr, nsamples, od.p,
                               [&](int q0, int ng, double* f) {
    SSNormals zd(z, zshard, 0, zshard, q0, ng, st0);
    return ss_post_paths(ss_stored(P), xsd.p, ns, w, ng, zd.p, zd.stride, 0, true, f);
  });
  if (rc) return rc;
  od.finish(st0);
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

// Building block for tests beside lmm_dev_statespace_interp: ONE latent from DEVICE pointers and given states, its mean not read.
// z: [sample][D W], f: [sample][ns].
int lmm_dev_statespace_post_sample(const double* x, int n, const lmm_gp_t* gp, const double* fstate, const double* sstate, const double* xs,
                                   int ns, const double* z, int nsamples, int chunk, double* f) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  std::shared_ptr<LatentSet> ls;
  const bool bad = !x || !gp || !fstate || !sstate || !xs || !z || !f || n <= 0 || ns < 1 || chunk < 0;
  if (int rc = ss_dev_prepare(bad, x, n, gp, ls, nsamples)) return rc;
  const Latent* lts = ls->lat.data();
  SSWindow w;
  if (int rc = ss_window(x, n, xs, ns, w)) return rc;
  const size_t zs = (size_t)ss_latent_dim(lts[0]) * w.W;
  return ss_for_sample_groups(std::max(w.W, ns), 1, nsamples, [&](int q0, int ng) {
    return ss_post_paths(ss_stored(x, n, lts, fstate, sstate), xs, ns, w, ng, z + (size_t)q0 * zs, zs, chunk, false, f + (size_t)q0 * ns);
  });
  LMM_CATCH
}

// ---- predictive log density from the posterior object (DESIGN.md 4.18 "Predictive log density from the posterior object") --------
// log p(the queries' data | the training data) of the stored latents: the filter over the window's backward chain.  w, r: [latent][ns]
// on the device, over the sorted queries (+Inf: unobserved); lml: S.ms host values.  Returns with streams[0] drained.
static void ss_post_logpdf(const SSStored& S, const double* xsd, int ns, const SSWindow& win, const double* w, const double* r, int chunk,
                           double* lml) {
  SSLpdfArgs a0{};
  a0.x = S.x; a0.n = S.n; a0.xs = xsd; a0.ns = ns; a0.src = win.src.p; a0.first = win.first; a0.W = win.W;
  ss_scored_scan(S.lts, S.ms, win.W, chunk, a0, launch_ss_post_logpdf, lml, [&](SSLpdfArgs& a, int k0, int nb) {
    for (int j = 0; j < nb; ++j) {
      ss_fill_lat(a.lat[j], S.lts[k0 + j], false);
      a.lat[j].fstate = S.fstate + S.off[k0 + j]; a.lat[j].sstate = S.sstate + S.off[k0 + j];
      a.lat[j].w = w + (size_t)(k0 + j) * ns; a.lat[j].r = r + (size_t)(k0 + j) * ns;
    }
  });
}

int lmm_oilmm_statespace_post_logpdf(const lmm_ss_post_t* post, const double* xs, int ns, const double* ys, double sigma2, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!post || !out || ns < 0) return fail(LMM_ERR_ARG, "bad arguments");
  if (g_f32) return ss_refuse_f32();
  if (!(sigma2 >= 0.0) || !std::isfinite(sigma2))
    return fail(LMM_ERR_ARG, "state-space posterior: sigma2 must be finite and > 0, or exactly 0 for the handle's own (sigma2 = %g)", sigma2);
  if (ns == 0) {
    *out = 0.0;
    return LMM_OK;
  }
  if (!xs || !ys) return fail(LMM_ERR_ARG, "bad arguments");
  const lmm_ss_post* P = post;
  const int p = P->p, m = P->m, ms = P->l1 - P->l0;
  const double s2 = sigma2 == 0.0 ? P->sigma2 : sigma2;
  const Latent* lts = P->ls->lat.data();
  hipStream_t st0 = g.streams[0];
  DevIn xsd(xs, (size_t)ns, st0), ysd(ys, (size_t)ns * p, st0);
  // every refusal comes before the smoothed states are touched
  SSWindow w;
  if (int rc = ss_window(P->x.p, P->n, xsd.p, ns, w)) return rc;
  SSFront Fr;
  if (int rc = ss_front(ysd.p, ns, p, P->U.data(), P->S.data(), m, s2, lts, P->l0, P->l1, Fr)) return rc;
  if (int rc = ss_post_ensure_smoothed(P, xsd.p, ns)) return rc;
  std::vector<double> lml(std::max(ms, 1), 0.0);
  ss_post_logpdf(ss_stored(P), xsd.p, ns, w, Fr.w.p, Fr.r.p, 0, lml.data());
  double value = 0.0;
  for (int j = 0; j < ms; ++j) value += lml[j];
  value += Fr.reg;
  *out = value;
  return LMM_OK;
  LMM_CATCH
}

// Building block for tests beside lmm_dev_statespace_post_sample: ONE latent from DEVICE pointers and given states, its mean not read
// (r is the residual).  w, r: ns values over the sorted queries (+Inf: unobserved); out: one value on the device.
int lmm_dev_statespace_post_logpdf(const double* x, int n, const lmm_gp_t* gp, const double* fstate, const double* sstate, const double* xs,
                                   int ns, const double* w, const double* r, int chunk, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  std::shared_ptr<LatentSet> ls;
  const bool bad = !x || !gp || !fstate || !sstate || !xs || !w || !r || !out || n <= 0 || ns < 1 || chunk < 0;
  if (int rc = ss_dev_prepare(bad, x, n, gp, ls)) return rc;
  SSWindow win;
  if (int rc = ss_window(x, n, xs, ns, win)) return rc;
  double h = 0.0;
  ss_post_logpdf(ss_stored(x, n, ls->lat.data(), fstate, sstate), xs, ns, win, w, r, chunk, &h);
  HIPCHK(hipMemcpyAsync(out, &h, sizeof(double), hipMemcpyHostToDevice, g.streams[0]));
  HIPCHK(hipStreamSynchronize(g.streams[0]));
  return LMM_OK;
  LMM_CATCH
}

extern "C" {

// Standard normals on the device (Philox4x32-10 + Box-Muller, Float64): out[j], j < count, reproducible for (seed, stream).
// out may be a host or a device pointer.  Optional companion of lmm_lmm_rand / lmm_lmm_rand_multi, whose normals are
// caller-supplied: the Julia shim draws them from the reference's rng on the host; this generator serves callers that do not
// need that stream (SURVEY.md section 8a, K7 "optional Philox").
int lmm_normals(unsigned long long seed, unsigned long long stream, size_t count, double* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!out && count > 0) return fail(LMM_ERR_ARG, "out is NULL");
  hipStream_t st0 = g.streams[0];
  DevOut od(out, count);
  launch_normals(seed, stream, count, od.p, st0);
  od.finish(st0);
  HIPCHK(hipStreamSynchronize(st0));
  return LMM_OK;
  LMM_CATCH
}

// ------------------------------------------------------------------------------------------------
// building blocks (device pointers) for tests / profiling
// ------------------------------------------------------------------------------------------------
int lmm_dev_potrf(double* A, int nrows, int ncols, int ld, double* Winv, int n_real, int* info_dev) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!A || !Winv || !info_dev || nrows % 64 || ncols % 64 || nrows < ncols || ld < nrows || (ld & 1))
    return fail(LMM_ERR_ARG, "bad arguments");
  potrf_one(A, ld, nrows, ncols, Winv, n_real, info_dev, g.streams[0]);
  int hinfo = 0;
  HIPCHK(hipMemcpyAsync(&hinfo, info_dev, sizeof(int), hipMemcpyDeviceToHost, g.streams[0]));
  HIPCHK(hipStreamSynchronize(g.streams[0]));
  // a dependency-wait timeout is an error of the launch (LMM_ERR_HIP); a non-positive pivot stays in *info_dev for the caller, as before
  if (hinfo == LMM_INFO_SYNC_TIMEOUT) return check_info(&hinfo, 1, 0);
  return LMM_OK;
  LMM_CATCH
}

// lmm_dev_potrf with the caller's zero extents (lmm_emul.h; device, nrows / 64 ints: per 64-row block the number of leading columns
// that hold +0 in all of its rows -- any lower bound of the true extents is valid, 0 everywhere leaves nothing out); zext = NULL is
// lmm_dev_potrf.  With LMM_ZERO_EXTENTS=0 / lmm_dev_set_zero_extents(0) the extents are ignored.
int lmm_dev_potrf_zext(double* A, int nrows, int ncols, int ld, double* Winv, int n_real, int* info_dev, const int* zext) {
  if (!zext) return lmm_dev_potrf(A, nrows, ncols, ld, Winv, n_real, info_dev);
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!A || !Winv || !info_dev || nrows % 64 || ncols % 64 || nrows < ncols || ld < nrows || (ld & 1))
    return fail(LMM_ERR_ARG, "bad arguments");
  hipStream_t st = g.streams[0];
  int* zx = zero_ext_scratch(nrows, 1, st);      // the padded layout potrf_batch takes; nullptr: switched off or fp32
  if (zx) HIPCHK(hipMemcpyAsync(zx, zext, (size_t)(nrows / 64) * sizeof(int), hipMemcpyDeviceToDevice, st));
  Batch B; B.add(A, Winv, info_dev);
  potrf_batch(B, ld, nrows, ncols, n_real, st, -1, zx);
  int hinfo = 0;
  HIPCHK(hipMemcpyAsync(&hinfo, info_dev, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (hinfo == LMM_INFO_SYNC_TIMEOUT) return check_info(&hinfo, 1, 0);
  return LMM_OK;
  LMM_CATCH
}

// The training Gram launch of the per-latent path (latent_lmls: train_gram_args, one batched launch per run of equal kinds) for nb
// latents gp[0 .. nb) on the caller's device memory: matrix j (nrows x ncols, ld; nrows, ncols multiples of 64, ncols >= n) at
// A + j * ld * ncols with the diagonal term noise[j] -- or noisevec (device, [nb][n]) -- and the nrider rider rows rider[j] (device,
// [nb][nrider][n]).  zext (host, [nb][nrows / 64]): the zero extents the launch kept (LMM_ZERO_EXT_NONE = 0x7F7F7F7F for a row block
// that is all zeros); all -1 when the switch is off or the compute dtype is Float32 (no extents are kept).
int lmm_dev_train_gram(double* A, int ld, int nrows, int ncols, const double* x, int d, int n, const lmm_gp_t* gp, int nb, const double* noise,
                       const double* noisevec, const double* rider, int nrider, int* zext) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!A || !x || !gp || !zext || (!noise && !noisevec) || nb < 1 || nb > LMM_MAX_BATCH || nrows % 64 || ncols % 64 || (ld & 1) || ld < nrows || ncols < n || n < 1 ||
      nrows < ncols || nrider < 0 || nrows - ncols < nrider || (nrider > 0 && !rider))
    return fail(LMM_ERR_ARG, "bad arguments");
  std::shared_ptr<LatentSet> ls;
  if (int rc = resolve(gp, nb, d, ls)) return rc;
  hipStream_t st = g.streams[0];
  Dims D(n, nrider);
  D.NC = ncols; D.NR = nrows; D.ld = ld;
  int* zx = zero_ext_scratch(nrows, nb, st);
  const int zld = zero_ext_ld(nrows);
  GramArgs ga[LMM_MAX_BATCH];
  for (int j = 0; j < nb; ++j) {
    ga[j] = train_gram_args(ls->lat[j], x, d, n, D, A + (size_t)j * ld * ncols, noisevec ? 0.0 : noise[j], noisevec ? noisevec + (size_t)j * n : nullptr,
                            rider ? rider + (size_t)j * nrider * n : nullptr, nrider);
    if (zx) { ga[j].zext = zx + (size_t)j * zld; ga[j].zext_ld = zld; }
  }
  gram_batch_g(ga, nb, st);
  std::vector<int> h((size_t)nb * zld, -1);
  if (zx) HIPCHK(hipMemcpyAsync(h.data(), zx, h.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int j = 0; j < nb; ++j)
    for (int r = 0; r < nrows / 64; ++r) zext[(size_t)j * (nrows / 64) + r] = h[(size_t)j * zld + r];
  return LMM_OK;
  LMM_CATCH
}

// The back substitution of a gradient or posterior pass on its own: exactly launch_backsolve, on the main stream.
int lmm_dev_backsolve(const double* L, size_t l_stride, int ld, const double* W, size_t w_stride, int nblk, double* z, size_t z_stride,
                      int nb) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!L || !W || !z || nblk < 1 || nb < 1 || nb > LMM_MAX_BATCH || ld < nblk * 64 || (ld & 1) || (l_stride & 1) ||
      (nb > 1 && z_stride < (size_t)nblk * 64))
    return fail(LMM_ERR_ARG, "lmm_dev_backsolve: bad arguments");
  BatchPtr Lb{}, Wb{}, zb{};
  for (int j = 0; j < nb; ++j) {
    Lb.p[j] = const_cast<double*>(L) + (size_t)j * l_stride; Wb.p[j] = const_cast<double*>(W) + (size_t)j * w_stride;
    zb.p[j] = z + (size_t)j * z_stride;
  }
  launch_backsolve(Lb, ld, Wb, nblk, zb, nb, g.streams[0]);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(g.streams[0]));
  return LMM_OK;
  LMM_CATCH
}

// The inverse of a gradient pass on its own, as KernelGradPass::launch queues it: R = identity, R <- L^-T (upper triangular), then
// lower(A) = R R' = Kt^-1 over the factor.
int lmm_dev_factor_inverse(double* A, size_t a_stride, int ld, int NC, const double* W, size_t w_stride, double* R, size_t r_stride,
                           int nb) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  const size_t mat = (size_t)ld * (NC > 0 ? NC : 0);
  if (!A || !W || !R || NC < 64 || NC % 64 || nb < 1 || nb > LMM_MAX_BATCH || ld < NC || (ld & 1) || (a_stride & 1) || (r_stride & 1) ||
      (nb > 1 && (a_stride < mat || r_stride < mat || w_stride < (size_t)NC * 64)))
    return fail(LMM_ERR_ARG, "lmm_dev_factor_inverse: bad arguments");
  hipStream_t st = g.streams[0];
  BatchPtr Ab{}, Wb{}, Rb{};
  for (int j = 0; j < nb; ++j) {
    Ab.p[j] = A + (size_t)j * a_stride; Wb.p[j] = const_cast<double*>(W) + (size_t)j * w_stride; Rb.p[j] = R + (size_t)j * r_stride;
    launch_set_identity(Rb.p[j], ld, NC, st);
  }
  trsm_rec(Rb, ld, NC, Ab, ld, Wb, nb, 0, NC, st, true);
  launch_syrk_upper_set(Ab, ld, Rb, ld, NC, nb, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(g.streams[0]));
  return LMM_OK;
  LMM_CATCH
}

// The region kernel's row-task plan for one block column (host arithmetic only; no device, no lmm_init needed).
int lmm_dev_region_plan(int P, int nb, int rows_below, int rows_real, int cus, int assistants, int out[3]) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!out || P < 1 || P > LMM_REGION_MAX_PANELS || nb < 1 || nb > LMM_MAX_BATCH || rows_below < 0 || rows_real > rows_below || cus < 1 || assistants < 0) {
    return fail(LMM_ERR_ARG, "lmm_dev_region_plan: bad arguments");
  }
  region_plan_probe(P, nb, rows_below, rows_real, cus, assistants, out);
  return LMM_OK;
}
// Test hook of the dataflow kernels' launch-epoch counter: *old_epoch (may be NULL) = the current value; set_to >= 0 replaces it (set
// it to 2^26 - 2 and the next launches execute the wrap-around clear of the persistent flag words).
int lmm_dev_flag_epoch(int set_to, int* old_epoch) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (set_to >= (1 << 26)) return fail(LMM_ERR_ARG, "lmm_dev_flag_epoch: the epoch has 26 bits");
  const int old = region_flag_epoch(set_to);
  if (old_epoch) *old_epoch = old;
  return LMM_OK;
}
// The allocation-extent guard on a freshly pooled block of alloc_bytes: LMM_OK when a rows x cols block of doubles with leading
// dimension ld fits, LMM_ERR_ARG (and nothing launched) when it does not.  Exists so that the guard itself has a test.
int lmm_dev_extent_check(size_t alloc_bytes, size_t rows, size_t ld, size_t cols) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  Buf<double> blk((alloc_bytes + 7) / 8);
  guard_extent(blk.p, rows, ld, cols, false, "lmm_dev_extent_check");
  return LMM_OK;
  LMM_CATCH
}

// Host-only (no GPU, no lmm_init needed): the status the library derives from `count` pivot-info words -- LMM_OK, LMM_ERR_NOT_PD
// (first non-zero word; lmm_last_error_detail gives latent_begin + index and the pivot) or LMM_ERR_HIP when ANY word carries the
// region kernel's dependency-timeout marker (-7777), whichever position it is in.  Exists so that this translation has a test.
int lmm_dev_check_info(const int* info, int count, int latent_begin) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!info || count < 0) return fail(LMM_ERR_ARG, "bad arguments");
  return check_info(info, (size_t)count, latent_begin);
}

// Test hook of the emulation switches (the env values are read once): on < 0 goes back to the env defaults.
int lmm_dev_set_f64_emul(int on, int min_k, int nmod) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (on < 0) { g_switches.emul_on = -1; g_switches.emul_mink = -1; g_switches.emul_nmod = LMM_EMUL_MAXMOD; return LMM_OK; }
  if (min_k < 128 || nmod < LMM_EMUL_MINMOD || nmod > LMM_EMUL_MAXMOD) return fail(LMM_ERR_ARG, "lmm_dev_set_f64_emul: min_k >= 128, %d <= nmod <= %d", LMM_EMUL_MINMOD, LMM_EMUL_MAXMOD);
  g_switches.emul_on = on ? 1 : 0; g_switches.emul_mink = min_k; g_switches.emul_nmod = nmod;
  return LMM_OK;
}
// Test hook of the f64 updates' screen (the env values LMM_F64_SCREEN, LMM_F64_SCREEN_MINK, LMM_F64_SCREEN_ROUNDS are read once):
// on = 0 / 1; every update on the f64 kernel with K >= min_k >= 128 and more than one tile column is screened, whatever its size
// (f64_screen_pays is off, as with an explicit LMM_F64_SCREEN_MINK); on < 0 goes back to the defaults (on, K >= 512, launches of more
// than one round).
int lmm_dev_set_f64_screen(int on, int min_k) {
  std::lock_guard<std::mutex> lk(g_mu);
  (void)factor_switches();      // the environment first, so that a later first read does not undo this
  if (on < 0) { const FactorSwitches d; g_switches.f64_screen = d.f64_screen; g_switches.f64_screen_mink = d.f64_screen_mink; g_switches.f64_screen_rounds = d.f64_screen_rounds; return LMM_OK; }
  if (min_k < 128) return fail(LMM_ERR_ARG, "lmm_dev_set_f64_screen: min_k >= 128");
  g_switches.f64_screen = on ? 1 : 0; g_switches.f64_screen_mink = min_k; g_switches.f64_screen_rounds = 0;
  return LMM_OK;
}
// Test hook of the zero extents (LMM_ZERO_EXTENTS, read once): on = 0 / 1; on < 0 goes back to the default (on).
int lmm_dev_set_zero_extents(int on) {
  std::lock_guard<std::mutex> lk(g_mu);
  (void)factor_switches();
  g_switches.zero_extents = on < 0 ? FactorSwitches().zero_extents : (on ? 1 : 0);
  return LMM_OK;
}
// Test hook of the size gate (LMM_ZERO_EXTENTS_MINCOLS, read once): a per-latent logpdf keeps extents for matrices of more than `cols`
// columns; cols < 0 goes back to the default (2048).
int lmm_dev_set_zero_extents_min_cols(int cols) {
  std::lock_guard<std::mutex> lk(g_mu);
  (void)factor_switches();
  g_switches.zero_extents_min_cols = cols < 0 ? FactorSwitches().zero_extents_min_cols : cols;
  return LMM_OK;
}
// Test hook: on != 0 makes every factorisation that was given zero extents count its void work items and copy the counters to the
// host when its launches are issued (that synchronises its stream).  out (may be NULL when cap = 0): 7 ints per region, update + leaf
// and emulated update + leaf step of the LAST factorisation of this process, in launch order: step kind (PotrfStepKind), j0, h, N, M,
// the count, and a shape word (region: its 128-row row tasks; update: 1 fused bulk rows + 2 x its strip mode).  The count: row tasks of a region launch that returned at entry; rest and column-0 items of an f64 update launch that did
// (a split tile once); 256 x 256 tiles the emulation's screen marked without reading C, all matrices of the batch together.  Empty
// when that factorisation had no extents.  Returns the number of steps (those beyond cap are counted, not written).
int lmm_dev_zero_extent_stats(int on, int* out, int cap) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (cap < 0 || (cap > 0 && !out)) return -fail(LMM_ERR_ARG, "lmm_dev_zero_extent_stats: bad arguments");
  g_zero_ext_stats = on ? 1 : 0;
  const int n = (int)(g_zero_ext_last.size() / 7);
  for (int i = 0; i < n && i < cap; ++i)
    for (int q = 0; q < 7; ++q) out[7 * i + q] = g_zero_ext_last[7 * i + q];
  return n;
}
// Test hook: FactorSwitches.deterministic (LMM_DETERMINISTIC, read once): no split-K atomics in the update launches.
int lmm_dev_set_deterministic(int on) {
  std::lock_guard<std::mutex> lk(g_mu);
  (void)factor_switches();
  g_switches.deterministic = on ? 1 : 0;
  return LMM_OK;
}
// Test hook: on != 0 makes every factorisation copy its screened updates' counters to the host when its launches are issued (that
// synchronises its stream).  out (may be NULL when cap = 0): 5 ints per screened update of the LAST factorisation of this process, in
// launch order: M, N, K, dead tiles the screen counted, 1 when the screen did its work (0: the vote made it return at entry).
// Returns the number of screened updates (those beyond cap are counted, not written).
int lmm_dev_f64_screen_stats(int on, int* out, int cap) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (cap < 0 || (cap > 0 && !out)) return -fail(LMM_ERR_ARG, "lmm_dev_f64_screen_stats: bad arguments");
  g_f64_screen_stats = on ? 1 : 0;
  const int n = (int)(g_f64_screen_last.size() / 5);
  for (int i = 0; i < n && i < cap; ++i)
    for (int q = 0; q < 5; ++q) out[5 * i + q] = g_f64_screen_last[5 * i + q];
  return n;
}
// Scan + screen of ONE f64 update shape on the caller's device memory, as a screened step of a factorisation runs them: C (M x N, ldc;
// the region), A (M x K, lda; its panel, whose first N rows are the B operand).  flags (host, MT x NT bytes, MT = ceil(M / 128), NT =
// ceil(N / 128); row-major over (tile row, tile column)): the bytes of the rest tiles 1 <= tj <= ti as the screen stored them, 0xFF
// elsewhere.  *dead = the count the screen kept.
int lmm_dev_f64_screen_flags(const double* C, int ldc, const double* A, int lda, int M, int N, int K, unsigned char* flags, int* dead) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!C || !A || !flags || !dead || ldc < M || lda < M || M < N || N <= 128 || M < 256 || K < 128 || (K % 128) != 0 || K > 16384) return fail(LMM_ERR_ARG, "bad arguments");
  guard_extent(C, M, ldc, N, false, "lmm_dev_f64_screen_flags (C)"); guard_extent(A, M, lda, K, false, "lmm_dev_f64_screen_flags (A)");
  const size_t fb = f64_screen_flag_bytes(M, N, POTRF_STRIP_NONE, 1);
  unsigned char* dflags = reinterpret_cast<unsigned char*>(call_scratch(fb / 8));
  int* stat = reinterpret_cast<int*>(call_scratch(1));
  unsigned long long* amax = reinterpret_cast<unsigned long long*>(call_scratch((size_t)M));
  hipStream_t st = g.streams[0];
  HIPCHK(hipMemsetAsync(dflags, 0xFF, fb, st));
  HIPCHK(hipMemsetAsync(stat, 0, 2 * sizeof(int), st));
  BatchPtr Cb{}, Pb{};
  Cb.p[0] = const_cast<double*>(C); Pb.p[0] = const_cast<double*>(A);
  EmulAmaxKeep keep{amax, M, 0, 0, {}, 0, nullptr, 0, 0};
  HIPCHK(launch_f64_screen(Cb, 0, ldc, Pb, 0, lda, M, N, K, POTRF_STRIP_NONE, 1, keep, dflags, stat, nullptr, st));
  const int MT = (M + 127) / 128, NT = (N + 127) / 128;
  HIPCHK(hipMemcpyAsync(flags, dflags, (size_t)MT * NT, hipMemcpyDeviceToHost, st));
  int hs[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(hs, stat, sizeof(hs), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  *dead = hs[0];
  return LMM_OK;
  LMM_CATCH
}
// Test hook of the shape rule that decides when nothing explicit is set (emul_pays): updates with K >= min_k_always are emulated, those
// with min_k_shape <= K < min_k_always when nb * outputs >= min_outputs; min_k_always < 0 goes back to the defaults.
int lmm_dev_set_f64_emul_rule(int min_k_always, int min_k_shape, double min_outputs) {
  g.err.clear();
  if (min_k_always < 0) { g_switches.rule_always = kRuleAlways; g_switches.rule_shape = kRuleShape; g_switches.rule_outs = kRuleOuts; return LMM_OK; }
  if (min_k_shape < 128 || min_k_always < min_k_shape || !(min_outputs >= 0.0)) return fail(LMM_ERR_ARG, "lmm_dev_set_f64_emul_rule: 128 <= min_k_shape <= min_k_always, min_outputs >= 0");
  g_switches.rule_always = min_k_always; g_switches.rule_shape = min_k_shape; g_switches.rule_outs = min_outputs;
  return LMM_OK;
}
// Test hook: at most g matrices per group of an emulated update (0: as many as the scratch block holds).  Results do not depend on it.
int lmm_dev_set_emul_group(int gcap) {
  g.err.clear();
  if (gcap < 0) return fail(LMM_ERR_ARG, "lmm_dev_set_emul_group: g >= 0");
  g_switches.emul_group_cap = gcap;
  return LMM_OK;
}
// Test hook: on = 0 makes every emulated update of a factorisation scan its whole panel for the row maxima, as if no earlier update
// had kept any; the default, 1, reads what earlier updates kept (emul_amax_cover).  Results do not depend on it.
int lmm_dev_set_emul_amax_reuse(int on) {
  g.err.clear();
  g_switches.emul_amax_reuse = on ? 1 : 0;
  return LMM_OK;
}
// Host-only (no GPU, no lmm_init needed): the emulation side of the plan potrf_batch makes for nb matrices of NR rows and NC columns.
// out[0] = bytes of the scratch block it asks for (0: nothing is emulated), out[1] = the G that block is sized for; then 6 words per
// trailing update with at least 128 columns, in launch order: M, N, K, emulated (0 / 1), matrices per group, scratch bytes at that
// group size (0, 0 when not emulated).  Returns the number of updates (records beyond cap are counted, not written), or -LMM_ERR_ARG.
int lmm_dev_emul_plan(int NR, int NC, int nb, long long* out, int cap) {
  g.err.clear();
  if (!out || cap < 0 || nb < 1 || nb > LMM_MAX_BATCH || NC < 128 || (NC % 64) != 0 || NR < NC) return -fail(LMM_ERR_ARG, "lmm_dev_emul_plan: bad arguments");
  const PotrfPlan P = emul_view(NR, NC, nb);
  out[0] = (long long)P.emul_bytes; out[1] = P.emul_G;
  for (size_t i = 0; i < P.updates.size() && i < (size_t)cap; ++i) {
    const PotrfUpdate& u = P.updates[i];
    long long* r = out + 2 + 6 * i;
    r[0] = u.M; r[1] = u.N; r[2] = u.K; r[3] = u.emulated; r[4] = u.group; r[5] = (long long)u.scratch;
  }
  return (int)P.updates.size();
}
// Host-only (no GPU, no lmm_init needed): what potrf_batch launches for nb matrices of NR rows and NC columns (rows_real of them holding
// data, -1: all) with in_flight batches running side by side on a device of cus CUs, in the compute dtype f32 != 0 / Float64, with
// strict progress on or off, under the current switches.  The layout of out is documented in include/lmm_hip.h.
int lmm_dev_potrf_plan(int NR, int NC, int nb, int rows_real, int in_flight, int cus, int f32, int strict, long long* out, int cap) {
  g.err.clear();
  if (!out || cap < 0 || nb < 1 || nb > LMM_MAX_BATCH || NC < 64 || (NC % 64) != 0 || (NR % 64) != 0 || NR < NC || rows_real > NR || rows_real < -1 ||
      (rows_real >= 0 && rows_real < NC) || in_flight < 1 || cus < 1)
    return -fail(LMM_ERR_ARG, "lmm_dev_potrf_plan: bad arguments");
  const PotrfPlan P = plan_potrf(NR, NC, nb, rows_real, in_flight, cus, f32 != 0, false, strict != 0, true, factor_switches());
  out[0] = P.panel128; out[1] = P.region_cols; out[2] = (long long)P.w2_doubles; out[3] = (long long)P.node_flag_ints;
  out[4] = (long long)P.asst_doubles; out[5] = (long long)P.emul_bytes; out[6] = P.emul_G; out[7] = P.emul_nmod;
  for (size_t i = 0; i < P.steps.size() && i < (size_t)cap; ++i) {
    const PotrfStep& s = P.steps[i];
    long long* r = out + LMM_POTRF_PLAN_HEADER + LMM_POTRF_PLAN_STEP * i;
    r[0] = s.kind; r[1] = s.j0; r[2] = s.h; r[3] = s.N; r[4] = s.M; r[5] = s.cls; r[6] = s.named();
    memcpy(&r[7], &s.work, 8); memcpy(&r[8], &s.bytes, 8);
    r[9] = s.first_done; r[10] = s.fused_bulk; r[11] = s.strip; r[12] = s.kind == POTRF_UPDATE_LEAF ? (long long)s.screened : s.group; r[13] = (long long)s.scratch;
  }
  return (int)P.steps.size();
}
// Test hook: at most wgs workgroups in the persistent grid of the emulation's GEMM (0: the default, one per CU), so that a small shape
// makes one workgroup walk several tiles.
int lmm_dev_set_emul_gemm_workgroups(int wgs) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (wgs < 0) return fail(LMM_ERR_ARG, "lmm_dev_set_emul_gemm_workgroups: wgs >= 0");
  emul_set_gemm_workgroups(wgs);
  return LMM_OK;
}
// Switch of the emulation GEMM's zero skip: 1 (the default, or LMM_EMUL_ZERO_SKIP unset) walks only the K blocks that are live in
// both operands of a tile, 0 (LMM_EMUL_ZERO_SKIP=0) walks all of them with the same kernel; on < 0 goes back to the env default.
// Results do not depend on it.
int lmm_dev_set_emul_zero_skip(int on) {
  std::lock_guard<std::mutex> lk(g_mu);
  emul_set_zero_skip(on);
  return LMM_OK;
}
// Test hook (default 0, never set outside tests): on != 0 fills the residue scratch of every group of an emulated update with a
// non-zero byte before its convert, in place of whatever an earlier update left in the blocks the convert no longer writes.
int lmm_dev_set_emul_scratch_poison(int on) {
  std::lock_guard<std::mutex> lk(g_mu);
  emul_set_scratch_poison(on);
  return LMM_OK;
}
// Host-only (no GPU, no lmm_init needed): the stage list of a GEMM tile whose operands have the live masks a (a0: K blocks 0 .. 63, a1:
// 64 .. 127) and b, at depth nk = K / 128 blocks, walked with the helpers the kernel's staging cursor uses (lmm_emul.h).  out[0 .. min(
// cap, length)) = the K blocks in walk order; *count (may be NULL) = what the kernel's MFMA loop takes for the length.  Returns the
// length of the walk, or -LMM_ERR_ARG.
int lmm_dev_emul_stage_list(unsigned long long a0, unsigned long long a1, unsigned long long b0, unsigned long long b1, int nk, int* out, int cap, int* count) {
  g.err.clear();
  if (nk < 1 || nk > 128 || cap < 0 || (cap > 0 && !out)) return -fail(LMM_ERR_ARG, "lmm_dev_emul_stage_list: 1 <= nk <= 128, cap >= 0");
  EmulMask m = emul_live_stages(EmulMask{a0, a1}, EmulMask{b0, b1}, nk);
  if (count) *count = emul_mask_count(m);
  int n = 0;
  for (; !emul_mask_empty(m); m = emul_mask_pop(m), ++n)
    if (n < cap) out[n] = emul_mask_first(m);
  return n;
}
// Switch of the emulation's screen (lmm_emul.h, negligible updates): 1 (the default, or LMM_EMUL_SCREEN unset) skips, in the GEMM and
// the combine, the tiles whose update cannot change a bit of C; 0 (LMM_EMUL_SCREEN=0) makes every tile live and the live id list the
// identity, with the same kernels; on < 0 goes back to the env default.  Results do not depend on it.
int lmm_dev_set_emul_screen(int on) {
  std::lock_guard<std::mutex> lk(g_mu);
  emul_set_screen(on);
  return LMM_OK;
}
// Test hook: the number of live tiles (of the trapezoid's tile list) in the last lmm_dev_syrk_emul call, -1 before the first.
static int g_emul_last_live_tiles = -1;
int lmm_dev_emul_last_live_tiles(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  return g_emul_last_live_tiles;
}
// Host-only (no GPU, no lmm_init needed): the screen's predicate (emul_negligible, lmm_emul.h) for `count` outputs of an update of
// depth K: out[i] = 1 when an output with the value c[i], whose two panel rows have the largest |entry| rowmax_i[i] and rowmax_j[i],
// is negligible -- the update cannot change a bit of it -- else 0.  Signs of the maxima are ignored; a NaN counts as above everything.
int lmm_dev_emul_negligible(int K, const double* rowmax_i, const double* rowmax_j, const double* c, int count, int* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (count < 0 || (count > 0 && (!rowmax_i || !rowmax_j || !c || !out)) || K < 1 || K > 16384) return fail(LMM_ERR_ARG, "lmm_dev_emul_negligible: bad arguments");
  for (int i = 0; i < count; ++i) {
    unsigned long long ri, rj;
    memcpy(&ri, &rowmax_i[i], 8); memcpy(&rj, &rowmax_j[i], 8);
    out[i] = emul_negligible(K, ri & 0x7FFFFFFFFFFFFFFFull, rj & 0x7FFFFFFFFFFFFFFFull, c[i]) ? 1 : 0;
  }
  return LMM_OK;
}
// C (M x N, lower trapezoid i >= j) -= A A[0:N]' through the emulation kernels: one matrix, device pointers.
int lmm_dev_syrk_emul(double* C, int ldc, const double* A, int lda, int M, int N, int K, int nmod) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!C || !A || nmod < LMM_EMUL_MINMOD || nmod > LMM_EMUL_MAXMOD || ldc < M || lda < M || !emul_shape_ok(M, N, K)) return fail(LMM_ERR_ARG, "bad arguments");
  guard_extent(C, M, ldc, N, false, "lmm_dev_syrk_emul (C)"); guard_extent(A, M, lda, K, false, "lmm_dev_syrk_emul (A)");
  const size_t bytes = emul_scratch_bytes(M, N, K, 1, nmod);
  double* scratch = call_scratch((bytes + 7) / 8);
  BatchPtr Cb{}, Pb{};
  Cb.p[0] = C; Pb.p[0] = const_cast<double*>(A);
  void* aux = call_scratch(emul_aux(M, 1, K).total_bmax / 8);      // no factorisation around it: the block maxima live there too
  const EmulScreen S = emul_screen_layout(M, N, 1, nmod);
  char* screen = reinterpret_cast<char*>(call_scratch(S.total / 8));
  guard_extent(screen, S.total / 8, S.total / 8, 1, false, "lmm_dev_syrk_emul (screen)");
  HIPCHK(launch_emul_update(Cb, 0, ldc, Pb, 0, lda, M, N, K, 1, 1, nmod, scratch, aux, screen, g.streams[0]));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(g.streams[0]));
  int counts[2] = {0, 0};
  HIPCHK(hipMemcpy(counts, screen + S.count, sizeof(counts), hipMemcpyDeviceToHost));
  g_emul_last_live_tiles = counts[1];
  return LMM_OK;
  LMM_CATCH
}
// Host-only (no GPU, no lmm_init needed): row scaling, residues, integer products modulo each modulus and the CRT combine of one
// small product in plain C++, with the constants and the scalar steps the kernels use (lmm_emul.h).
int lmm_dev_emul_host(const double* A, int lda, const double* B, int ldb, int M, int N, int K, int nmod, int k_bound, double* out,
                      int ldo, double* consts) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!A || !B || !out || M < 1 || N < 1 || K < 1 || K > 4096 || lda < M || ldb < N || ldo < M || nmod < LMM_EMUL_MINMOD || nmod > LMM_EMUL_MAXMOD || k_bound < K)
    return fail(LMM_ERR_ARG, "lmm_dev_emul_host: bad arguments");
  const EmulConst c = emul_make_const(nmod);
  const int bits = emul_bits(nmod, k_bound);
  struct Rows { std::vector<int8_t> res; std::vector<double> sc; std::vector<int> ex; };
  auto convert = [&](const double* X, int ld, int n) {
    Rows r; r.res.assign((size_t)nmod * n * K, 0); r.sc.assign(n, 0.0); r.ex.assign(n, 0);
    for (int i = 0; i < n; ++i) {
      double amax = 0.0; bool finite = true;
      for (int k = 0; k < K; ++k) { const double a = std::fabs(X[i + (size_t)k * ld]); if (!(a <= 1.79769313486231570815e308)) finite = false; else if (a > amax) amax = a; }
      if (!finite) { r.sc[i] = std::nan(""); continue; }
      if (amax == 0.0) continue;
      const int e = emul_row_exp(amax);
      r.sc[i] = 1.0; r.ex[i] = e - bits;
      for (int k = 0; k < K; ++k) {
        const long long v = emul_trunc(X[i + (size_t)k * ld], bits - e);
        int res[LMM_EMUL_MAXMOD];
        emul_residues<LMM_EMUL_MAXMOD>(v, res);
        for (int t = 0; t < nmod; ++t) r.res[((size_t)t * n + i) * K + k] = (int8_t)res[t];
      }
    }
    return r;
  };
  const Rows ra = convert(A, lda, M), rb = convert(B, ldb, N);
  for (int j = 0; j < N; ++j)
    for (int i = 0; i < M; ++i) {
      int u[LMM_EMUL_MAXMOD] = {0};
      for (int t = 0; t < nmod; ++t) {
        int acc = 0;
        for (int k = 0; k < K; ++k) acc += (int)ra.res[((size_t)t * M + i) * K + k] * (int)rb.res[((size_t)t * N + j) * K + k];
        u[t] = (int)(int8_t)emul_acc_residue(acc, emul_fold_const(c.p[t]), (float)c.p[t], 1.0f / (float)c.p[t]);
      }
      out[i + (size_t)j * ldo] = std::ldexp(emul_crt(u, c) * ra.sc[i] * rb.sc[j], ra.ex[i] + rb.ex[j]);
    }
  if (consts) {      // [0..15] p_t, [16..31] w_t1, [32..47] w_t2, [48..63] w_t3, [64..66] P1..P3, [67] b
    for (int t = 0; t < LMM_EMUL_MAXMOD; ++t) { consts[t] = c.p[t]; consts[16 + t] = c.w1[t]; consts[32 + t] = c.w2[t]; consts[48 + t] = c.w3[t]; }
    consts[64] = c.P1; consts[65] = c.P2; consts[66] = c.P3; consts[67] = bits;
  }
  return LMM_OK;
}
// Host-only (no GPU, no lmm_init needed): the convert kernel's residue step (emul_residues, lmm_emul.h) on `count` integers, |v| <= 2^58:
// out[i nmod + t] = the int8 residue of v[i] modulo the t-th modulus.  exhaustive (may be NULL, 2 words): the reduction step
// (emul_reduce_odd) run on every x it can see, for every odd modulus and both signs -- [0] = the number of (modulus, x) cases, [1] = how
// many of them gave a result that is not congruent to +-x or lies outside [-(p - 1) / 2, (p - 1) / 2].
int lmm_dev_emul_residues(const long long* v, int count, int nmod, signed char* out, long long* exhaustive) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (count < 0 || (count > 0 && (!v || !out)) || nmod < LMM_EMUL_MINMOD || nmod > LMM_EMUL_MAXMOD) return fail(LMM_ERR_ARG, "lmm_dev_emul_residues: bad arguments");
  for (int i = 0; i < count; ++i) {
    if (v[i] > (1ll << LMM_EMUL_MAXBITS) || v[i] < -(1ll << LMM_EMUL_MAXBITS)) return fail(LMM_ERR_ARG, "lmm_dev_emul_residues: |v| <= 2^%d", LMM_EMUL_MAXBITS);
    int res[LMM_EMUL_MAXMOD];
    emul_residues<LMM_EMUL_MAXMOD>(v[i], res);
    for (int t = 0; t < nmod; ++t) out[(size_t)i * nmod + t] = (signed char)(int8_t)res[t];
  }
  if (exhaustive) {
    long long cases = 0, bad = 0;
    for (int t = 1; t < LMM_EMUL_MAXMOD; ++t) {
      const int p = kEmulModuli[t], half = (p - 1) / 2;
      for (int x = 0; x <= kEmulDot.xmax[t]; ++x, ++cases) {
        const int rp = emul_reduce_odd(LMM_EMUL_MAGIC_BITS + (unsigned)x, 1.0f, t), rn = emul_reduce_odd(LMM_EMUL_MAGIC_BITS + (unsigned)x, -1.0f, t);
        if ((rp - x) % p != 0 || rp < -half || rp > half || (rn + x) % p != 0 || rn < -half || rn > half) ++bad;
      }
    }
    exhaustive[0] = cases; exhaustive[1] = bad;
  }
  return LMM_OK;
}
// Host-only (no GPU, no lmm_init needed): the convert's liveness decision (emul_block_live, lmm_emul.h) for `count` (row, K block)
// pairs at the bit budget `bits`: out[i] = 1 when a block whose largest |entry| is blockmax[i], in a row whose largest |entry| is
// rowmax[i], holds a truncated integer that is not zero, else 0.  Signs are ignored; a NaN counts as above everything, as in the scan.
int lmm_dev_emul_block_live(const double* rowmax, const double* blockmax, int count, int bits, int* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (count < 0 || (count > 0 && (!rowmax || !blockmax || !out)) || bits < 1 || bits > LMM_EMUL_MAXBITS) return fail(LMM_ERR_ARG, "lmm_dev_emul_block_live: bad arguments");
  for (int i = 0; i < count; ++i) {
    unsigned long long r, b;
    memcpy(&r, &rowmax[i], 8); memcpy(&b, &blockmax[i], 8);
    out[i] = emul_block_live(r & 0x7FFFFFFFFFFFFFFFull, b & 0x7FFFFFFFFFFFFFFFull, bits) ? 1 : 0;
  }
  return LMM_OK;
}
// Host-only (no GPU, no lmm_init needed): the GEMM epilogue's reduction (emul_acc_residue, lmm_emul.h) of `count` int32 accumulators,
// |x| <= 2^28: out[i nmod + t] = the int8 residue of x[i] modulo the t-th modulus.  exhaustive (may be NULL, 2 words): the float step
// (emul_fold_reduce) run on every value y of the folded accumulator it can see, |y| <= emul_acc_fold_max, for every modulus -- [0] = the
// number of (modulus, y) cases, [1] = how many gave a byte that is not y's residue in [-(p - 1) / 2, (p - 1) / 2] ([-128, 127] for 256).
int lmm_dev_emul_acc_residues(const int* x, int count, int nmod, signed char* out, long long* exhaustive) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (count < 0 || (count > 0 && (!x || !out)) || nmod < LMM_EMUL_MINMOD || nmod > LMM_EMUL_MAXMOD) return fail(LMM_ERR_ARG, "lmm_dev_emul_acc_residues: bad arguments");
  for (int i = 0; i < count; ++i) {
    if (x[i] > (1 << 28) || x[i] < -(1 << 28)) return fail(LMM_ERR_ARG, "lmm_dev_emul_acc_residues: |x| <= 2^28");
    for (int t = 0; t < nmod; ++t) {
      const int p = kEmulModuli[t];
      out[(size_t)i * nmod + t] = (signed char)(int8_t)emul_acc_residue(x[i], emul_fold_const(p), (float)p, 1.0f / (float)p);
    }
  }
  if (exhaustive) {
    long long cases = 0, bad = 0;
    for (int t = 0; t < LMM_EMUL_MAXMOD; ++t) {
      const int p = kEmulModuli[t], lo = -(p / 2), ymax = emul_acc_fold_max(emul_fold_const(p));
      for (int y = -ymax; y <= ymax; ++y, ++cases) {
        const int r = (int)(int8_t)emul_fold_reduce(LMM_EMUL_MAGIC_BITS + (unsigned)y, (float)p, 1.0f / (float)p);
        if ((r - y) % p != 0 || r < lo || r > lo + p - 1) ++bad;
      }
    }
    exhaustive[0] = cases; exhaustive[1] = bad;
  }
  return LMM_OK;
}

int lmm_dev_gemm_nt_sub(double* C, int ldc, const double* A, int lda, const double* B, int ldb, int M, int N, int K,
                        int lower) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!C || !A || !B || M <= 0 || N <= 0 || K <= 0 || M % 64 || N % 64 || K % 16 || (ldc & 1) || (lda & 1) || (ldb & 1) || ldc < M || lda < M || ldb < N)
    return fail(LMM_ERR_ARG, "bad arguments");
  // lower: the tile enumeration (MT - tj row tiles under column tile tj of a common-origin region) assumes a trapezoid at least as
  // tall as it is wide
  if (lower && M < N) return fail(LMM_ERR_ARG, "lower != 0 needs M >= N (lower trapezoid of a common-origin region)");
  launch_gemm_nt(C, ldc, A, lda, B, ldb, M, N, K, lower, false, g.streams[0]);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(g.streams[0]));
  return LMM_OK;
  LMM_CATCH
}

int lmm_dev_gram(double* A, int ld, int nrows, int ncols, const double* x, int d, int n, const lmm_gp_t* gp,
                 double diag_add) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!A || !x || !gp || nrows % 64 || ncols % 64 || (ld & 1) || ld < nrows) return fail(LMM_ERR_ARG, "bad arguments");
  GramArgs a{};
  a.A = A; a.ld = ld; a.nrows = nrows; a.ncols = ncols; a.x = x; a.d = d; a.n = n;
  std::shared_ptr<LatentSet> ls;
  if ((gp->kind >> 8) || (gp->kind & LMM_KERNEL_BASE_MASK) == LMM_KERNEL_SHO) {      // a tagged latent: resolve its tag like the entry points do; an SHO latent: d = 1 is checked there
    if (int rc = resolve(gp, 1, d, ls)) return rc;
    ls->lat[0].set_kernel(a);
  } else plain_latent(*gp).set_kernel(a);
  a.diag_add = diag_add; a.pad_diag = 1.0;
  gram_g(a, g.streams[0]);
  HIPCHK(hipStreamSynchronize(g.streams[0]));
  return LMM_OK;
  LMM_CATCH
}

int lmm_profile_begin(int serial) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  g.prof = true; g.prof_serial = serial != 0;
  g.prof_recs.clear();
  return LMM_OK;
}

int lmm_profile_end(lmm_prof_entry_t* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!out) return fail(LMM_ERR_ARG, "out is NULL");
  HIPCHK(hipDeviceSynchronize());
  for (int c = 0; c < LMM_PROF_COUNT; ++c) { out[c].launches = 0; out[c].ms = 0.0; out[c].work = 0.0; out[c].bytes = 0.0; }
  for (auto& r : g.prof_recs) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, r.e0, r.e1));
    out[r.cls].launches += r.count; out[r.cls].ms += ms; out[r.cls].work += r.work; out[r.cls].bytes += r.bytes;
    if (getenv("LMM_PROF_DUMP") && r.M > 0)
      fprintf(stderr, "[prof] cls=%d M=%d N=%d K=%d ms=%.4f tflops=%.2f\n", r.cls, r.M, r.N, r.K, ms, r.work / (ms * 1e-3) / 1e12);
    g.ev_pool.push_back(r.e0); g.ev_pool.push_back(r.e1);
  }
  g.prof_recs.clear();
  g.prof = false; g.prof_serial = false;
  return LMM_OK;
  LMM_CATCH
}

// Write-only yardstick for the Gram assembly's roofline line: GB/s of hipMemsetAsync into a pooled block of `bytes` (median-free mean
// of `reps` back-to-back fills between two events on the main stream, after one untimed fill that touches the block).
int lmm_dev_write_rate(size_t bytes, int reps, double* gbs) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  if (!gbs || bytes < (1u << 20) || reps < 1) return fail(LMM_ERR_ARG, "bad arguments");
  Buf<double> blk(bytes / 8);
  hipStream_t st = g.streams[0];
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
  HIPCHK(hipMemsetAsync(blk.p, 0, bytes, st));
  HIPCHK(hipEventRecord(e0, st));
  for (int r = 0; r < reps; ++r) HIPCHK(hipMemsetAsync(blk.p, 0, bytes, st));
  HIPCHK(hipEventRecord(e1, st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  *gbs = (double)bytes * reps / (ms * 1e-3) / 1e9;
  return LMM_OK;
  LMM_CATCH
}

int lmm_dev_mfma_f64_peak(double* tflops) {
  std::lock_guard<std::mutex> lk(g_mu);
  REQUIRE_INIT();
  LMM_TRY
  const int blocks = 256 * 2, iters = 5000;
  Buf<double> out((size_t)blocks * 256);
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
  launch_mfma_peak(out.p, blocks, iters, g.streams[0]);   // warm-up of the same length (clock ramp)
  HIPCHK(hipEventRecord(e0, g.streams[0]));
  launch_mfma_peak(out.p, blocks, iters, g.streams[0]);
  HIPCHK(hipEventRecord(e1, g.streams[0]));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  const double flops = (double)blocks * 4 /*waves*/ * iters * 16.0 * 2048.0;      // 16 MFMAs of 16 x 16 x 4 x 2 flops per iteration
  *tflops = flops / (ms * 1e-3) / 1e12;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return LMM_OK;
  LMM_CATCH
}

}  // extern "C"
