// C-ABI of the MI355X TZDDPC hot path (see include/tzddpc.h).  Host side: has tz_plan.h plan the problem
// (orderings, 4x4 MFMA patches, Gram work plan, ELL tables, LDS placement), uploads the plan's tables and
// launches the kernels of tz_kernels.hip.h on one HIP stream.  No torch types, no CPU compute fallback: every
// numeric result comes out of a kernel.
#include "tz_kernels.hip.h"
#include "tz_sample.hip.h"
#include "tz_plan.h"

// Neither build of the library reads an environment variable: what a caller may choose goes through tz_problem_desc (plan_flags)
// and the tz_problem_set_* entry points.  The diagnostic build (libtzddpc_hip_prof.so, -DTZ_PROFILE=1) only adds per-phase clocks.
#include "../../include/tzddpc.h"

#include <memory>

static thread_local std::string g_err;

#define TZ_FAIL(code, ...) TZ_FAIL_TO(g_err, code, __VA_ARGS__)
#define TZ_HIP(call) do { hipError_t _e = (call); if (_e != hipSuccess) { \
    char _b[512]; snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
    g_err = _b; return TZ_ERR_HIP; } } while (0)

namespace {

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t count) {
    if (p) { (void)hipFree(p); p = nullptr; }
    n = count;
    if (count == 0) return hipSuccess;
    return hipMalloc((void**)&p, count * sizeof(T));
  }
  hipError_t upload(const T* src, size_t count) {
    hipError_t e = alloc(count);
    if (e != hipSuccess || count == 0) return e;
    return hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
  }
  hipError_t upload(const std::vector<T>& v) { return upload(v.data(), v.size()); }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};

// device copy of a lane-ELL table of the plan (TzEll in tz_ipm.hip.h)
struct DevEll {
  DevBuf<TzEllEnt> ent; DevBuf<int> seg; DevBuf<double> val; DevBuf<unsigned short> idx;
  int L = 1, VL = 0;
  hipError_t upload(const TzEllTable& t) {
    L = t.L; VL = t.VL;
    hipError_t e;
    if ((e = ent.upload(t.ent)) != hipSuccess || (e = val.upload(t.val)) != hipSuccess || (e = idx.upload(t.idx)) != hipSuccess) return e;
    return seg.upload(t.seg);
  }
  TzEll view() const { return TzEll{L, VL, ent.p, seg.p, val.p, idx.p}; }
};

struct DevCsr {          // device copy of an affine map of the plan (TzCsr)
  DevBuf<TzEllEnt> ent;
  DevBuf<double> c0;
  int rows = 0, W = 1;
  hipError_t upload(const TzMapTable& t) {
    rows = t.rows; W = t.W;
    hipError_t e = ent.upload(t.ent);
    return e != hipSuccess ? e : c0.upload(t.c0);
  }
  TzCsr view() const { return TzCsr{rows, W, ent.p, c0.p}; }
};

// What a closed-loop step may start from: the previous step (x / s / lambda in the workspace, valid for prevB trajectories) or the
// stored start (tz_problem_store_start: solution and multipliers of one reference solve).
struct WarmState {
  int prevB = 0;                           // 0: nothing valid
  bool have_ref = false;
  DevBuf<double> ref_x, ref_lam;
  void invalidate() { prevB = 0; }
  void mark_valid(int B) { prevB = B; }
  bool valid_for(int B) const { return prevB == B; }
  void set_ref(bool on) { have_ref = on; if (on) invalidate(); }      // a new stored start replaces the previous step's solution
};

enum { K_TUBE = 0, K_IPM = 1, K_FINISH = 2, K_PLANT = 3, K_COUNT = 4 };

typedef void (*ipm_fn_t)(IpmParams);
// Kernel variants: <rows per thread, 64-column groups, workgroups per CU the register budget is compiled for>.
//   nz <= 64   (one column group): quad layout, single-wave Cholesky; always fits four workgroups per CU (128 registers).
//   nz  > 64   tile-triangle layout, blocked Gram, two-phase Cholesky (tz_tt.hip.h): 256 registers (two workgroups per CU) or
//              512 (one) -- the blocked Gram keeps an 8 x 8 block of tiles in accumulators.
//   more than 1024 rows (5 or 6 per thread): tile-triangle variants only.
template <int R> ipm_fn_t ipm_pick_tt(int ncg, int w) {
  if (w >= 2) { switch (ncg) { case 1: case 2: return tz_ipm_kernel<R, 2, 2>; case 3: return tz_ipm_kernel<R, 3, 2>; default: return tz_ipm_kernel<R, 4, 2>; } }
  switch (ncg) { case 1: case 2: return tz_ipm_kernel<R, 2, 1>; case 3: return tz_ipm_kernel<R, 3, 1>; default: return tz_ipm_kernel<R, 4, 1>; }
}
// The variant for a plan (tt: the plan's class); null when a development build does not carry it, TZ_NO_VARIANT says why.
ipm_fn_t ipm_kernel_for(int maxr, int ncg, int wgs_per_cu, bool tt) {
#ifdef TZ_ONLY_SMALL      // development builds (assembly study, quick A/B of the bench problem): only the variant for mi <= 256, nz <= 64
  (void)wgs_per_cu; (void)tt;
  return (maxr == 1 && ncg == 1) ? tz_ipm_kernel<1, 1, TZ_MINWAVES> : nullptr;
#elif defined(TZ_ONLY_TT)  // development builds of the tile-triangle class: -DTZ_ONLY_TT=R,NCG,W  (one variant, seconds to build)
#define TZ_NO_VARIANT "kernel class and table format disagree (development build?)"
  (void)maxr; (void)ncg; (void)wgs_per_cu;
  return tt ? tz_ipm_kernel<TZ_ONLY_TT> : nullptr;
#else
  if (!tt) {
    switch (maxr) { case 1: return tz_ipm_kernel<1, 1, TZ_MINWAVES>; case 2: return tz_ipm_kernel<2, 1, TZ_MINWAVES>; case 3: return tz_ipm_kernel<3, 1, TZ_MINWAVES>; default: return tz_ipm_kernel<4, 1, TZ_MINWAVES>; }
  }
  switch (maxr) {
    case 1: return ipm_pick_tt<1>(ncg, wgs_per_cu); case 2: return ipm_pick_tt<2>(ncg, wgs_per_cu); case 3: return ipm_pick_tt<3>(ncg, wgs_per_cu);
    case 4: return ipm_pick_tt<4>(ncg, wgs_per_cu);
    case 5: return ncg <= 3 ? tz_ipm_kernel<5, 3, 1> : tz_ipm_kernel<5, 4, 1>;
    default: return ncg <= 3 ? tz_ipm_kernel<6, 3, 1> : tz_ipm_kernel<6, 4, 1>;
  }
#endif
}
#ifndef TZ_NO_VARIANT
#define TZ_NO_VARIANT "this development build (TZ_ONLY_SMALL) carries only the mi <= 256, nz <= 64 kernel"
#endif

// "use this device": the entry points that take a device number start with it
int use_device(int device) {
  int ndev = 0;
  TZ_HIP(hipGetDeviceCount(&ndev));
  if (ndev <= 0) TZ_FAIL(TZ_ERR_HIP, "no HIP device visible: the TZDDPC hot path has no CPU fallback");
  if (device < 0 || device >= ndev) TZ_FAIL(TZ_ERR_INVALID, "device %d out of range (0..%d)", device, ndev - 1);
  TZ_HIP(hipSetDevice(device));
  return TZ_OK;
}

}  // namespace

struct tz_genstack {
  int device = 0, n = 0, m = 0, N = 0, nseg = 0, rec = 0, nchunk = 0;
  int64_t G = 0;
  std::vector<int> seg_ptr;                 // literal order
  DevBuf<double> recs_sorted, recs_lit, recs_mf, recs_mfn, c0, cE, cZ, K, partial, in_e0, in_zeta, o_c, o_rx, o_ru, o_Z;
  DevBuf<int> src_lit, seg_chunk_ptr;
  DevBuf<GsChunk> chunks;
  DevBuf<GsChunkM> chunks_m;                // matrix-core layout (tz_genstack_mfma_kernel): groups of 4 generators, K rows appended
  bool mfma = false;
  int rows_mf = 0;                          // rows per generator in recs_mf: n + m (K rows appended) or n (formed in the kernel)
  size_t pcap = 0;                          // doubles allocated for `partial`
  bool have_cZ = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

namespace {
int gs_inputs(tz_genstack* g, int B, const double* e0, const double* zeta, int mem, const double** de0, const double** dz) {
  const size_t p = g->n + g->m;
  if (mem == TZ_MEM_DEVICE) { *de0 = e0; *dz = zeta; return TZ_OK; }
  if (mem != TZ_MEM_HOST) TZ_FAIL(TZ_ERR_INVALID, "mem must be TZ_MEM_HOST or TZ_MEM_DEVICE");
  TZ_HIP(g->in_e0.upload(e0, (size_t)B * g->n)); TZ_HIP(g->in_zeta.upload(zeta, (size_t)B * g->N * p));
  *de0 = g->in_e0.p; *dz = g->in_zeta.p;
  return TZ_OK;
}

// room for the per-(chunk, trajectory) partial sums of gs_eval at batch size B (the narrow kernel writes TZ_GS_NARROW_SUB of them)
int gs_reserve_partial(tz_genstack* g, int B) {
  const size_t need = (size_t)std::max(g->nchunk, 1) * (B <= 64 ? TZ_GS_NARROW_SUB : 1) * B * (g->n + g->m);
  if (need > g->pcap) { TZ_HIP(g->partial.alloc(need)); g->pcap = need; }
  return TZ_OK;
}

// evaluation of the whole stack for B trajectories, device pointers, on `st`
int gs_eval(tz_genstack* g, int B, const double* de0, const double* dz, double* dc, double* drx, double* dru, hipStream_t st) {
  const int n = g->n, m = g->m, p = n + m;
  GenstackParams q{B, n, m, g->N, g->nseg, g->nchunk, g->rec, g->recs_sorted.p, g->chunks.p, g->K.p, de0, dz, g->partial.p};
  const dim3 grid((unsigned)g->nchunk, (unsigned)((B + 255) / 256));
  int nsub = 1;
  TZ_HIP(hipEventRecord(g->ev0, st));
  if (g->nchunk > 0 && g->mfma) {
    // few trajectories: every wave takes all of them and a quarter of the generators (the stack is streamed once: HBM-bound);
    // many: 256 per workgroup, the stack is re-read from L2 by the tiles of a chunk, which share an XCD
    const bool split = B <= 64;
    const int nq = B <= 16 ? 1 : (B <= 32 ? 2 : 4);
    nsub = split ? TZ_GS_NARROW_SUB : 1;
    const int ntt = split ? nsub : (B + 255) / 256;
    const bool krows = g->rows_mf == p || (B > 32 && B <= 64);       // which copy of the stack: K rows appended, or formed in the kernel
    GenstackMParams qm{B, n, m, g->N, g->nchunk, ntt, nsub, krows ? g->recs_mf.p : g->recs_mfn.p, g->K.p, g->chunks_m.p, de0, dz, g->partial.p};
    const dim3 gm((unsigned)(((g->nchunk + 7) / 8) * 8 * ntt));
#define TZ_GS_LAUNCH(RR, PP) do { \
      if (!split) hipLaunchKernelGGL((tz_genstack_mfma_kernel<RR, PP, 4>), gm, dim3(256), 0, st, qm); \
      else if (nq == 1) hipLaunchKernelGGL((tz_genstack_mfma_narrow_kernel<RR, PP, 1>), gm, dim3(256), 0, st, qm); \
      else if (nq == 2) hipLaunchKernelGGL((tz_genstack_mfma_narrow_kernel<RR, PP, 2>), gm, dim3(256), 0, st, qm); \
      else hipLaunchKernelGGL((tz_genstack_mfma_narrow_kernel<RR, PP, 4>), gm, dim3(256), 0, st, qm); } while (0)
#define TZ_GS_ROWS(PP) do { if (krows) TZ_GS_LAUNCH(PP, PP); else TZ_GS_LAUNCH(PP - 1, PP); } while (0)      // stored rows: n + m, or n (m = 1)
    switch (p) {
      case 3: TZ_GS_ROWS(3); break;
      case 4: TZ_GS_ROWS(4); break;
      case 5: TZ_GS_ROWS(5); break;
      case 6: TZ_GS_ROWS(6); break;
      default: TZ_GS_ROWS(7); break;
    }
#undef TZ_GS_ROWS
#undef TZ_GS_LAUNCH
  } else if (g->nchunk > 0) {
    if (n == 2 && m == 1) hipLaunchKernelGGL((tz_genstack_kernel<2, 1>), grid, dim3(256), 0, st, q);
    else if (n == 4 && m == 1) hipLaunchKernelGGL((tz_genstack_kernel<4, 1>), grid, dim3(256), 0, st, q);
    else if (n == 5 && m == 1) hipLaunchKernelGGL((tz_genstack_kernel<5, 1>), grid, dim3(256), 0, st, q);
    else hipLaunchKernelGGL((tz_genstack_kernel<0, 0>), grid, dim3(256), 0, st, q);
  }
  TZ_HIP(hipEventRecord(g->ev1, st));          // the stream kernel alone (what rocprofv3 reports for it); the reduction follows
  GsReduceParams r{B, n, m, g->N, g->nseg, nsub, g->seg_chunk_ptr.p, g->partial.p, g->c0.p, g->cE.p, g->have_cZ ? g->cZ.p : nullptr, de0, dz, dc, drx, dru};
  const size_t total = (size_t)B * g->nseg * p;
  if (B <= 64 && n <= 16) hipLaunchKernelGGL(tz_genstack_reduce16_kernel, dim3((unsigned)((total * 16 + 255) / 256)), dim3(256), 0, st, r);   // few trajectories: latency, not bytes
  else hipLaunchKernelGGL(tz_genstack_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, r);
  TZ_HIP(hipGetLastError());
  return TZ_OK;
}
}  // namespace

struct tz_problem {
  int device = 0;
  int n = 0, m = 0, N = 0, nz = 0, mi = 0, ntheta = 0, npar = 0, nc_rows = 0, pmax = 0;
  TzPlanSizes pl;              // derived sizes and decisions of the plan (tz_plan.h)
  int max_iter = 40;
  double tol = 1e-10, reg = 1e-12, step_frac = 0.99, cost_scale = 1.0, r0 = 0.0;
  // constants
  DevBuf<double> P, Gp, act_scale, Dz, Phi, Gam, r1, R2, CK, DK, K, CKpow, Ttube, par_lo, par_hi, rec0, recx, recy;
  DevBuf<int> power, row_of, klist, item_ptr, smask, shift_var, shift_row;
  DevBuf<double> shift_xs, shift_ls;
  int shift_policy = 0;        // 0 never, 1 always, k >= 2: after a step of >= k iterations (tz_problem_set_warm_shift)
  int shift_quiet = 16;        // leave the shifted regime after this many one-iteration shifted steps (0: never)
  bool have_shift = false;
  DevBuf<IpmItem> items;
  DevCsr q, h, par;
  DevEll eg, et;
  // workspace (capacity Bcap)
  int Bcap = 0;
  DevBuf<double> theta, qv, hv, x, s, lam, v, xbar, cost, in_x0, in_e0;
  DevBuf<int> prestatus, status, iters, sticky, prev_status, shift_state;
  DevBuf<uint8_t> active;
  // closed-loop state / plant (simulate)
  DevBuf<double> st_x, st_xbar, st_e, plantA, plantB, noise, xtraj, utraj, costtraj;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // timing
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool[K_COUNT];
  size_t ev_used[K_COUNT] = {0, 0, 0, 0};
  double t_ms[K_COUNT] = {0, 0, 0, 0};
  int64_t t_count[K_COUNT] = {0, 0, 0, 0};
  int lastB = 0;
  bool prof = TZ_PROFILE;      // diagnostic build: per-phase clocks of workgroup 0 (tz_debug_fetch item 6)
  WarmState warm;
  double warm_floor = 1e-8, warm_gain = 1.0, warm_cap = 1e300, mu_factor = 1e-3, res_factor = 100.0;
  DevBuf<TzGUnit> gunits; DevBuf<int> gunit_ptr;
  DevBuf<int> vpos;            // staircase ordering (tile-triangle class): device position of v[k, j]; null = identity
  std::vector<int> permc, permr;   // device variable / row i is the caller's permc[i] / permr[i] (identity without the staircase ordering)
  bool fuse_enabled = true;    // pl.fused, until a tube stack is attached
  struct tz_genstack* tube_stack = nullptr;   // literal problems: decision-independent generators, evaluated per solve (not owned)
  DevBuf<double> ts_zeta, ts_c, ts_rx, ts_ru;  int ts_cap = 0;
  void (*ipm_fn)(IpmParams) = nullptr;
  DevBuf<unsigned long long> prof_buf, work_buf;
};

__global__ void tz_seed_kernel(int B, int nz, int mi, const double* rx, const double* rl, double* x, double* lam, int* prev_status, int* iters, int* shift_state) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (size_t)B * nz) x[i] = rx[i % nz];
  if (i < (size_t)B * mi) lam[i] = rl[i % mi];
  if (i < (size_t)B) { prev_status[i] = 0; iters[i] = 0; shift_state[i] = -2; }      // -2: stored start (tz_ipm_kernel: taken unshifted, then the shifted regime)
}

namespace {

int ensure_workspace(tz_problem* p, int B) {
  if (B <= p->Bcap) return TZ_OK;
  TZ_HIP(hipSetDevice(p->device));
  size_t b = (size_t)B;
  TZ_HIP(p->theta.alloc(b * p->ntheta));
  TZ_HIP(p->qv.alloc(b * p->nz));
  TZ_HIP(p->hv.alloc(b * p->mi));
  TZ_HIP(p->x.alloc(b * p->nz));
  TZ_HIP(p->s.alloc(b * p->mi));
  TZ_HIP(p->lam.alloc(b * p->mi));
  TZ_HIP(p->v.alloc(b * p->N * p->m));
  TZ_HIP(p->xbar.alloc(b * (p->N + 1) * p->n));
  TZ_HIP(p->cost.alloc(b));
  TZ_HIP(p->in_x0.alloc(b * p->n));
  TZ_HIP(p->in_e0.alloc(b * p->n));
  TZ_HIP(p->prestatus.alloc(b));
  TZ_HIP(p->status.alloc(b));
  TZ_HIP(p->iters.alloc(b));
  TZ_HIP(p->sticky.alloc(b));
  TZ_HIP(p->prev_status.alloc(b));
  TZ_HIP(p->shift_state.alloc(b));
  TZ_HIP(hipMemset(p->shift_state.p, 0, b * sizeof(int)));
  TZ_HIP(p->active.alloc(b * std::max(p->nc_rows, 1)));
  TZ_HIP(p->st_x.alloc(b * p->n));
  TZ_HIP(p->st_xbar.alloc(b * p->n));
  TZ_HIP(p->st_e.alloc(b * p->n));
  p->Bcap = B;
  p->warm.invalidate();
  return TZ_OK;
}

void drain_timing_one(tz_problem* p, int k) {
  for (size_t i = 0; i < p->ev_used[k]; ++i) {
    float ms = 0.f;
    if (hipEventSynchronize(p->ev_pool[k][i].second) == hipSuccess &&
        hipEventElapsedTime(&ms, p->ev_pool[k][i].first, p->ev_pool[k][i].second) == hipSuccess) {
      p->t_ms[k] += ms; p->t_count[k]++;
    }
  }
  p->ev_used[k] = 0;
}

struct Timer {
  tz_problem* p; int k; hipEvent_t e0 = nullptr, e1 = nullptr;
  Timer(tz_problem* p_, int k_) : p(p_), k(k_) {
    if (!p->timing) return;
    if (p->ev_used[k] == p->ev_pool[k].size()) {
      if (p->ev_pool[k].size() >= 4096) drain_timing_one(p, k);       // pool exhausted: fold what is recorded (one stream sync)
      else {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
        p->ev_pool[k].push_back({a, b});
      }
    }
    e0 = p->ev_pool[k][p->ev_used[k]].first; e1 = p->ev_pool[k][p->ev_used[k]].second;
    p->ev_used[k]++;
    (void)hipEventRecord(e0, p->stream);
  }
  ~Timer() { if (e1) (void)hipEventRecord(e1, p->stream); }
};

void drain_timing(tz_problem* p) {
  for (int k = 0; k < K_COUNT; ++k) drain_timing_one(p, k);
}

IpmParams ipm_params(tz_problem* p, int B, int* d_status, int* d_iters, bool warm, bool track_prev) {
  IpmParams ip{};
  ip.B = B; ip.nz = p->nz; ip.mi = p->mi; ip.nzp = p->pl.nzp; ip.mip = p->pl.mip; ip.Tz = p->pl.Tz; ip.Kc = p->pl.Kc; ip.nquads = p->pl.nquads;
  ip.P = p->P.p; ip.Gp = p->Gp.p; ip.items = p->items.p; ip.item_ptr = p->item_ptr.p; ip.klist = p->klist.p; ip.smask = p->smask.p; ip.eg = p->eg.view(); ip.et = p->et.view(); ip.nell = p->pl.nell;
  ip.q = p->qv.p; ip.h = p->hv.p; ip.prestatus = p->prestatus.p; ip.x = p->x.p; ip.s = p->s.p; ip.lam = p->lam.p;
  ip.status = d_status; ip.iters = d_iters ? d_iters : p->iters.p;
  ip.max_iter = p->max_iter; ip.tol = p->tol; ip.reg = p->reg; ip.step_frac = p->step_frac; ip.mu_tol = p->tol * p->mu_factor; ip.tol_res = p->tol * p->res_factor;
  ip.inv_mi = 1.0 / p->mi; ip.mu_floor = 1e-3 * ip.mu_tol; ip.tol_loose = 1e3 * p->tol; ip.step_frac_retry = std::min(p->step_frac, 0.99);
  ip.prof = p->prof ? p->prof_buf.p : nullptr;
  ip.work = p->timing ? p->work_buf.p : nullptr;
  ip.TS = p->pl.TS; ip.ntile = p->pl.ntile; ip.gu = p->pl.gu; ip.gunits = p->gunits.p; ip.gunit_ptr = p->gunit_ptr.p;
  ip.nklist = p->pl.nklist; ip.nP = p->pl.nP; ip.ksplit = p->pl.ksplit ? 1 : 0; ip.ntube = p->pl.ntube;
  ip.shift_policy = p->have_shift ? p->shift_policy : 0; ip.shift_quiet = p->shift_quiet;
  ip.shift_state = p->shift_state.p;
  ip.sx = p->shift_var.p; ip.sr = p->shift_row.p; ip.sxs = p->shift_xs.p; ip.sls = p->shift_ls.p;
  ip.warm = warm ? 1 : 0; ip.warm_floor = p->warm_floor;
  ip.warm_gain = p->warm_gain; ip.warm_cap = p->warm_cap; ip.aff_thr = 0.99; ip.aff_mu = 1e-3;
  ip.prev_status = warm ? p->prev_status.p : nullptr;
  ip.status_copy = track_prev ? p->prev_status.p : nullptr;
  return ip;
}

// Launch blocks: the fields that come from the problem, by name; the launch sites add their pointers.
TubeParams tube_params(const tz_problem* p, int B) {
  TubeParams t{};
  t.B = B; t.n = p->n; t.m = p->m; t.N = p->N; t.pmax = p->pmax; t.ntheta = p->ntheta;
  t.CKpow = p->CKpow.p; t.T = p->Ttube.p; t.power = p->power.p;
  return t;
}

FinishParams finish_params(const tz_problem* p, int B) {
  FinishParams f{};
  f.B = B; f.n = p->n; f.m = p->m; f.N = p->N; f.nz = p->nz; f.mi = p->mi; f.nzp = p->pl.nzp; f.nc_rows = p->nc_rows;
  f.P = p->P.p; f.Dz = p->Dz.p; f.Phi = p->Phi.p; f.Gam = p->Gam.p; f.r1 = p->r1.p; f.R2 = p->R2.p; f.r0 = p->r0; f.cost_scale = p->cost_scale;
  f.row_of = p->row_of.p; f.act_scale = p->act_scale.p; f.vpos = p->vpos.p; f.rec0 = p->rec0.p; f.recx = p->recx.p; f.recy = p->recy.p;
  return f;
}

// What a closed-loop call reads and writes, all in device memory.  Element [b] of step t of a strided array is at
// base + b * stride + t * step.
struct ClosedLoopIO {
  double* x; double* xbar; double* e;                  // B x n each: the state, advanced in place
  const double* w; size_t w_stride, w_step;            // disturbances
  const double* A; const double* Bm;                   // the plant: n x n, n x m ...
  size_t A_stride, B_stride;                           // ... of the batch (0), or one per trajectory (n n, n m: the *_plants entry points)
  double* u_out; size_t u_stride, u_step;              // may be null
  double* x_out; size_t x_stride, x_step;              // may be null: copy of x+
  double* cost; size_t cost_stride, cost_step;         // cost_step 0: one slot per trajectory, overwritten by every step
  int* status;                                         // B: solver status of the step, overwritten by every step
  int* sticky;                                         // may be null; B: first non-zero status of the run
  bool sticky_fresh;                                   // the run clears sticky itself (the caller has not)
  bool fresh;                                          // a loop of its own (tz_simulate_batch): starts without a previous step and marks none
};

PlantParams plant_params(const tz_problem* p, int B, const ClosedLoopIO& io) {        // step 0; v and xbar_pred stay null (fused step)
  PlantParams q{};
  q.B = B; q.n = p->n; q.m = p->m; q.N = p->N; q.K = p->K.p; q.A = io.A; q.Bm = io.Bm; q.A_stride = io.A_stride; q.B_stride = io.B_stride;
  q.w = io.w; q.w_stride = io.w_stride; q.status = io.status; q.x = io.x; q.xbar = io.xbar; q.e = io.e;
  q.u_out = io.u_out; q.u_stride = io.u_stride; q.x_out = io.x_out; q.x_stride = io.x_stride; q.sticky = io.sticky;
  return q;
}

// literal problems: theta from the attached generator stack
int tube_stack_theta(tz_problem* p, int B, const double* d_e0, hipStream_t st) {
  tz_genstack* g = p->tube_stack;
  const int n = p->n, m = p->m, pq = n + m;
  if (B > p->ts_cap) {
    TZ_HIP(p->ts_zeta.alloc((size_t)B * g->N * pq)); TZ_HIP(hipMemset(p->ts_zeta.p, 0, (size_t)B * g->N * pq * sizeof(double)));
    TZ_HIP(p->ts_c.alloc((size_t)B * g->nseg * n)); TZ_HIP(p->ts_rx.alloc((size_t)B * g->nseg * n)); TZ_HIP(p->ts_ru.alloc((size_t)B * g->nseg * m));
    p->ts_cap = B;
  }
  if (int rcp = gs_reserve_partial(g, B)) return rcp;
  int rc = gs_eval(g, B, d_e0, p->ts_zeta.p, p->ts_c.p, p->ts_rx.p, p->ts_ru.p, st);
  if (rc) return rc;
  ThetaStackParams q{B, n, m, p->N, g->nseg, p->ntheta, p->ts_c.p, p->ts_rx.p, p->ts_ru.p, p->theta.p};
  const size_t total = (size_t)B * p->N * (2 * n + m);
  hipLaunchKernelGGL(tz_theta_stack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, q);
  TZ_HIP(hipGetLastError());
  return TZ_OK;
}

// Core launch sequence on device-resident inputs: tube -> affine -> ipm -> finish.
int launch_solve(tz_problem* p, int B, const double* d_xbar0, const double* d_e0,
                 double* d_v, double* d_xbar, double* d_cost, int* d_status, int* d_iters, uint8_t* d_active, size_t cost_stride = 1, bool warm = false, bool track_prev = false) {
  hipStream_t st = p->stream;
  p->lastB = B;
  {
    Timer tm(p, K_TUBE);
    TubeParams tp = tube_params(p, B);
    tp.xbar0 = d_xbar0; tp.e0 = d_e0; tp.theta = p->theta.p; tp.prestatus = p->prestatus.p;
    hipLaunchKernelGGL(tz_tube_kernel, dim3(B), dim3(64), 0, st, tp);
    if (p->tube_stack) { int rc = tube_stack_theta(p, B, d_e0, st); if (rc) return rc; }
    AffineParams ap{B, p->ntheta, p->nz, p->mi, p->npar, p->q.view(), p->h.view(), p->par.view(), p->par_lo.p, p->par_hi.p,
                    p->theta.p, p->qv.p, p->hv.p, p->prestatus.p};
    size_t total = (size_t)B * (p->nz + p->mi + p->npar);
    hipLaunchKernelGGL(tz_affine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ap);
  }
  {
    Timer tm(p, K_IPM);
    IpmParams ip = ipm_params(p, B, d_status, d_iters, warm, track_prev);
    // active-set readout (slack < multiplier) needs the complementarity products well below the slacks: three decades below the
    // stopping target, but never below 1e-6 tol (1e-16 at the default tolerance) -- an unbounded 1e-3 under a tight stopping target
    // asked degenerate problems for mu = 1e-18 and they ended TZ_NUMERICAL
    if (d_active) { const double f = std::min(1.0, std::max(1e-3, 1e-6 * p->tol / ip.mu_tol)); ip.mu_tol *= f; ip.mu_floor *= f; }
    hipLaunchKernelGGL(p->ipm_fn, dim3(B), dim3(TZ_THREADS), p->pl.lds_bytes, st, ip);
  }
  {
    Timer tm(p, K_FINISH);
    FinishParams fp = finish_params(p, B);
    fp.xbar0 = d_xbar0; fp.q = p->qv.p; fp.x = p->x.p; fp.s = p->s.p; fp.lam = p->lam.p; fp.status = d_status;
    fp.v = d_v; fp.xbar = d_xbar; fp.cost = d_cost; fp.active = d_active; fp.cost_stride = cost_stride;
    hipLaunchKernelGGL(tz_finish_kernel, dim3(B), dim3(64), 0, st, fp);
  }
  TZ_HIP(hipGetLastError());
  return TZ_OK;
}

// What a closed-loop launch starts from: the previous step's solution; else the stored start, seeded into every trajectory (the solution
// of ONE reference solve, tz_problem_store_start: the caller's point, typically the centre of X0 with e0 = 0); else the cold point.
int closed_loop_warm(tz_problem* p, int B, bool* warm) {
  const bool prev = p->warm.valid_for(B);
  *warm = prev || p->warm.have_ref;
  if (prev || !p->warm.have_ref) return TZ_OK;
  const size_t total = (size_t)B * std::max(p->nz, p->mi);
  hipLaunchKernelGGL(tz_seed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, p->stream, B, p->nz, p->mi, p->warm.ref_x.p, p->warm.ref_lam.p,
                     p->x.p, p->lam.p, p->prev_status.p, p->iters.p, p->shift_state.p);
  TZ_HIP(hipGetLastError());
  p->warm.mark_valid(B);
  return TZ_OK;
}

// K closed-loop steps of B trajectories: what tz_mpc_step, tz_mpc_run and tz_simulate_batch do once their arguments are on the device.
// Fused: ONE launch of tz_ipm_kernel with F.on does tube, parameter maps, interior point, recovery / objective and plant update of all
// K steps; theta, q and h never reach HBM and the state never leaves the workgroup.  Otherwise launch_solve and tz_plant_kernel per
// step: same arithmetic, four kernels.
int run_closed_loop(tz_problem* p, int B, int K, const ClosedLoopIO& io) {
  if (io.fresh) p->warm.invalidate();
  bool warm = false;
  if (int rc = closed_loop_warm(p, B, &warm)) return rc;
  if (p->fuse_enabled) {
    p->lastB = B;
    Timer tm(p, K_IPM);
    IpmParams ip = ipm_params(p, B, io.status, p->iters.p, warm, true);
    FuseParams& F = ip.F;
    F.on = 1; F.npar = p->npar; F.ntheta = p->ntheta; F.lean_epilogue = p->pl.lean_epilogue ? 1 : 0; F.sticky_fresh = io.sticky_fresh ? 1 : 0;
    F.nsteps = K; F.warm_steps = 1; ip.warm_steps = F.warm_steps;
    F.w_step = io.w_step; F.u_step = io.u_step; F.x_step = io.x_step; F.cost_step = io.cost_step;
    F.tube = tube_params(p, B); F.tube.xbar0 = io.xbar; F.tube.e0 = io.e;                   // theta stays in LDS
    F.qmap = p->q.view(); F.hmap = p->h.view(); F.parmap = p->par.view(); F.par_lo = p->par_lo.p; F.par_hi = p->par_hi.p;
    F.fin = finish_params(p, B);
    F.fin.xbar0 = io.xbar; F.fin.status = io.status; F.fin.cost = io.cost; F.fin.cost_stride = io.cost_stride;
    if (K == 1) { F.fin.v = p->v.p; F.fin.xbar = p->xbar.p; }                                // a single step also leaves its prediction
    F.plant = plant_params(p, B, io);
    hipLaunchKernelGGL(p->ipm_fn, dim3(B), dim3(TZ_THREADS), p->pl.lds_bytes, p->stream, ip);
    TZ_HIP(hipGetLastError());
  } else {
    if (io.sticky && io.sticky_fresh) TZ_HIP(hipMemsetAsync(io.sticky, 0, (size_t)B * sizeof(int), p->stream));
    for (int t = 0; t < K; ++t) {
      if (int rc = launch_solve(p, B, io.xbar, io.e, p->v.p, p->xbar.p, io.cost + t * io.cost_step, io.status, p->iters.p, nullptr, io.cost_stride, warm || t > 0, true)) return rc;
      Timer tm(p, K_PLANT);
      PlantParams pp = plant_params(p, B, io);
      pp.v = p->v.p; pp.xbar_pred = p->xbar.p; pp.w += t * io.w_step;          // v and the prediction launch_solve left in the workspace
      if (pp.u_out) pp.u_out += t * io.u_step;
      if (pp.x_out) pp.x_out += t * io.x_step;
      hipLaunchKernelGGL(tz_plant_kernel, dim3((B + 63) / 64), dim3(64), 0, p->stream, pp);
      TZ_HIP(hipGetLastError());
    }
  }
  if (!io.fresh) p->warm.mark_valid(B);
  return TZ_OK;
}

}  // namespace

extern "C" {

int tz_abi_version(void) { return TZ_ABI_VERSION; }
const char* tz_last_error(void) { return g_err.c_str(); }

int tz_device_count(int* count) {
  if (!count) TZ_FAIL(TZ_ERR_INVALID, "count is null");
  TZ_HIP(hipGetDeviceCount(count));
  return TZ_OK;
}

int tz_identify_batch(int device, int32_t B, int32_t T, int32_t n, int32_t m, const double* u, const double* x,
                      const double* w_center, const double* K, int32_t k_shared,
                      double* C, double* s, double* sK, double* CK, int32_t* status, int mem) {
  if (!u || !x || !w_center || !C || !s || !status) TZ_FAIL(TZ_ERR_INVALID, "null argument");
  if (B <= 0 || T < 2) TZ_FAIL(TZ_ERR_INVALID, "B must be positive and T at least 2");
  if (n < 1 || n > TZ_ID_NMAX || m < 1 || m > TZ_ID_MMAX) TZ_FAIL(TZ_ERR_UNSUPPORTED, "identification on the device (K0): dim_x must be 1..%d and dim_u 1..%d", TZ_ID_NMAX, TZ_ID_MMAX);
  if (K && (!sK || !CK)) TZ_FAIL(TZ_ERR_INVALID, "sK and CK are required when K is given");
  if (mem != TZ_MEM_HOST && mem != TZ_MEM_DEVICE) TZ_FAIL(TZ_ERR_INVALID, "mem must be TZ_MEM_HOST or TZ_MEM_DEVICE");
  if (int rc = use_device(device)) return rc;
  const int p = n + m;
  const size_t b = (size_t)B;
  IdentifyParams q{B, T, n, m, u, x, w_center, K, k_shared ? 1 : 0, C, s, K ? sK : nullptr, K ? CK : nullptr, status};
  DevBuf<double> du, dx, dw, dK, dC, ds, dsK, dCK; DevBuf<int> dst;
  if (mem == TZ_MEM_HOST) {
    TZ_HIP(du.upload(u, b * T * m)); TZ_HIP(dx.upload(x, b * T * n)); TZ_HIP(dw.upload(w_center, (size_t)n));
    if (K) TZ_HIP(dK.upload(K, (k_shared ? 1 : b) * m * n));
    TZ_HIP(dC.alloc(b * n * p)); TZ_HIP(ds.alloc(b * p)); TZ_HIP(dsK.alloc(b * n)); TZ_HIP(dCK.alloc(b * n * n)); TZ_HIP(dst.alloc(b));
    q.u = du.p; q.x = dx.p; q.wc = dw.p; q.K = K ? dK.p : nullptr; q.C = dC.p; q.s = ds.p; q.sK = K ? dsK.p : nullptr; q.CK = K ? dCK.p : nullptr; q.status = dst.p;
  }
  hipLaunchKernelGGL(tz_identify_kernel, dim3(B), dim3(64), 0, 0, q);
  TZ_HIP(hipGetLastError());
  if (mem == TZ_MEM_HOST) {
    TZ_HIP(hipMemcpy(C, dC.p, b * n * p * sizeof(double), hipMemcpyDeviceToHost));
    TZ_HIP(hipMemcpy(s, ds.p, b * p * sizeof(double), hipMemcpyDeviceToHost));
    if (K) { TZ_HIP(hipMemcpy(sK, dsK.p, b * n * sizeof(double), hipMemcpyDeviceToHost)); TZ_HIP(hipMemcpy(CK, dCK.p, b * n * n * sizeof(double), hipMemcpyDeviceToHost)); }
    TZ_HIP(hipMemcpy(status, dst.p, b * sizeof(int), hipMemcpyDeviceToHost));
  }
  return TZ_OK;
}

// ---- gain synthesis (tz_gain.hip.h): spectral radii of sampled closed loops, CCP ascent of ||A + B K||_F ------------------------
static int gain_batch(bool adversary, int device, int32_t S, int32_t n, int32_t ngen, const double* M0, const double* H,
                      const double* beta, int32_t max_iter, double* beta_out, double* val, int32_t* aux) {
  if (!M0 || !beta || !val || !aux || (ngen > 0 && !H) || (adversary && !beta_out)) TZ_FAIL(TZ_ERR_INVALID, "null argument");
  if (S <= 0 || ngen < 0) TZ_FAIL(TZ_ERR_INVALID, "S must be positive, ngen non-negative");
  if (n < 1 || n > TZ_GN_NMAX) TZ_FAIL(TZ_ERR_UNSUPPORTED, "dim_x must be 1..%d", TZ_GN_NMAX);
  if (adversary && max_iter < 1) TZ_FAIL(TZ_ERR_INVALID, "max_iter must be positive");
  if (int rc = use_device(device)) return rc;
  const size_t s = (size_t)S, g = (size_t)ngen, n2 = (size_t)n * n;
  DevBuf<double> dM0, dH, dbeta, dbout, dval; DevBuf<int> daux;
  TZ_HIP(dM0.upload(M0, n2));
  if (g) { TZ_HIP(dH.upload(H, g * n2)); TZ_HIP(dbeta.upload(beta, s * g)); } else { TZ_HIP(dH.alloc(1)); TZ_HIP(dbeta.alloc(1)); }
  TZ_HIP(dval.alloc(s)); TZ_HIP(daux.alloc(s));
  if (adversary) TZ_HIP(dbout.alloc(std::max<size_t>(s * g, 1)));
  GainParams q{S, n, ngen, max_iter, dM0.p, dH.p, dbeta.p, adversary ? dbout.p : nullptr, dval.p, daux.p};
  const dim3 grid((S + 63) / 64), block(64);
  if (adversary) hipLaunchKernelGGL(tz_adversary_kernel, dim3(S), dim3(256), 0, 0, q);          // one workgroup per starting point, lane = generator
  else hipLaunchKernelGGL(tz_specrad_kernel, grid, block, 0, 0, q);
  TZ_HIP(hipGetLastError());
  TZ_HIP(hipMemcpy(val, dval.p, s * sizeof(double), hipMemcpyDeviceToHost));
  TZ_HIP(hipMemcpy(aux, daux.p, s * sizeof(int), hipMemcpyDeviceToHost));
  if (adversary && g) TZ_HIP(hipMemcpy(beta_out, dbout.p, s * g * sizeof(double), hipMemcpyDeviceToHost));
  return TZ_OK;
}

int tz_specrad_batch(int device, int32_t S, int32_t n, int32_t ngen, const double* M0, const double* H, const double* beta,
                     double* rho, int32_t* status) {
  return gain_batch(false, device, S, n, ngen, M0, H, beta, 0, nullptr, rho, status);
}

int tz_adversary_batch(int device, int32_t S, int32_t n, int32_t ngen, const double* M0, const double* H, const double* beta0,
                       int32_t max_iter, double* beta, double* fro, int32_t* steps) {
  return gain_batch(true, device, S, n, ngen, M0, H, beta0, max_iter, beta, fro, steps);
}

// ---- Monte Carlo over the model set (tz_sample.hip.h): plants of Mdata and disturbances of W, drawn on the device --------------
// The checks both entry points share; before the device query, so a machine without a GPU reports a bad call as such.
static int sample_check(int32_t B, int32_t ngen, const double* centre, const double* gen, int32_t mode, int64_t first, int mem) {
  if (!centre || (ngen > 0 && !gen)) TZ_FAIL(TZ_ERR_INVALID, "null argument");
  if (B <= 0 || ngen < 0 || first < 0) TZ_FAIL(TZ_ERR_INVALID, "B must be positive, ngen and first non-negative");
  if (ngen > TZ_SP_MAXGEN) TZ_FAIL(TZ_ERR_INVALID, "at most %d generators (24 bits of the counter carry the block index)", TZ_SP_MAXGEN);
  if (mode != TZ_SAMPLE_UNIFORM && mode != TZ_SAMPLE_VERTEX) TZ_FAIL(TZ_ERR_INVALID, "mode must be TZ_SAMPLE_UNIFORM or TZ_SAMPLE_VERTEX");
  if (mem != TZ_MEM_HOST && mem != TZ_MEM_DEVICE) TZ_FAIL(TZ_ERR_INVALID, "mem must be TZ_MEM_HOST or TZ_MEM_DEVICE");
  return TZ_OK;
}

// uploads centre and generators, fills the fields every launch shares, launches; q carries the item shape and the outputs
static int sample_launch(SampleParams q, uint64_t seed, int64_t first, const double* centre, const double* gen, int32_t mode,
                         DevBuf<double>& dc, DevBuf<double>& dg) {
  TZ_HIP(dc.upload(centre, (size_t)q.nout));
  if (q.ngen > 0) TZ_HIP(dg.upload(gen, (size_t)q.ngen * q.nout));
  q.key0 = (unsigned)(seed & 0xffffffffu); q.key1 = (unsigned)(seed >> 32); q.first = (unsigned long long)first;
  q.mode = mode == TZ_SAMPLE_VERTEX ? TZ_SP_VERTEX : TZ_SP_UNIFORM; q.centre = dc.p; q.gen = dg.p;
  const unsigned long long items = (unsigned long long)q.B * q.T;
  hipLaunchKernelGGL(tz_sample_kernel, dim3((unsigned)((items + TZ_SP_ITEMS - 1) / TZ_SP_ITEMS)), dim3(64 * TZ_SP_ITEMS), 0, 0, q);
  TZ_HIP(hipGetLastError());
  return TZ_OK;
}

int tz_sample_plants(int device, uint64_t seed, int64_t first, int32_t B, int32_t n, int32_t m, int32_t ngen,
                     const double* centre, const double* gen, int32_t mode, double* A_out, double* B_out, int mem) {
  if (!A_out || !B_out) TZ_FAIL(TZ_ERR_INVALID, "null argument");
  if (int rc = sample_check(B, ngen, centre, gen, mode, first, mem)) return rc;
  if (n < 1 || n > TZ_NMAX || m < 1 || m > TZ_MMAX) TZ_FAIL(TZ_ERR_INVALID, "dim_x must be 1..%d and dim_u 1..%d", TZ_NMAX, TZ_MMAX);
  if (int rc = use_device(device)) return rc;
  const size_t b = (size_t)B, nn = (size_t)n * n, nm = (size_t)n * m;
  DevBuf<double> dc, dg, dA, dB;
  SampleParams q{};
  q.B = B; q.T = 1; q.nout = n * (n + m); q.ngen = ngen; q.stream = 0; q.width = n + m; q.wA = n;
  q.out0 = A_out; q.s0 = nn; q.out1 = B_out; q.s1 = nm;
  if (mem == TZ_MEM_HOST) { TZ_HIP(dA.alloc(b * nn)); TZ_HIP(dB.alloc(b * nm)); q.out0 = dA.p; q.out1 = dB.p; }
  if (int rc = sample_launch(q, seed, first, centre, gen, mode, dc, dg)) return rc;
  if (mem == TZ_MEM_HOST) {
    TZ_HIP(hipMemcpy(A_out, dA.p, b * nn * sizeof(double), hipMemcpyDeviceToHost));
    TZ_HIP(hipMemcpy(B_out, dB.p, b * nm * sizeof(double), hipMemcpyDeviceToHost));
  } else TZ_HIP(hipDeviceSynchronize());          // centre / gen copies are freed on return
  return TZ_OK;
}

int tz_sample_noise(int device, uint64_t seed, int64_t first, int32_t B, int32_t T, int32_t n, int32_t ngen,
                    const double* centre, const double* gen, int32_t mode, size_t traj_stride, size_t step_stride,
                    double* out, int mem) {
  if (!out) TZ_FAIL(TZ_ERR_INVALID, "null argument");
  if (int rc = sample_check(B, ngen, centre, gen, mode, first, mem)) return rc;
  if (T <= 0) TZ_FAIL(TZ_ERR_INVALID, "T must be positive");
  if (n < 1 || n > TZ_NMAX) TZ_FAIL(TZ_ERR_INVALID, "dim_x must be 1..%d", TZ_NMAX);
  if ((unsigned long long)B * T > 0x7fffffffull) TZ_FAIL(TZ_ERR_INVALID, "B * T must stay below 2^31");
  // the two layouts that do not overlap: trajectory-major (B x T x n and wider) or step-major (T x B x n and wider)
  const bool traj_major = step_stride >= (size_t)n && traj_stride >= (size_t)T * step_stride;
  const bool step_major = traj_stride >= (size_t)n && step_stride >= (size_t)B * traj_stride;
  if (!traj_major && !step_major) TZ_FAIL(TZ_ERR_INVALID, "traj_stride / step_stride describe overlapping rows");
  if (int rc = use_device(device)) return rc;
  const size_t extent = (size_t)(B - 1) * traj_stride + (size_t)(T - 1) * step_stride + n;
  DevBuf<double> dc, dg, dout;
  SampleParams q{};
  q.B = B; q.T = T; q.nout = n; q.ngen = ngen; q.stream = 1; q.width = 0;
  q.out0 = out; q.s0 = traj_stride; q.st0 = step_stride;
  if (mem == TZ_MEM_HOST) { TZ_HIP(dout.upload(out, extent)); q.out0 = dout.p; }      // what lies between the rows is handed back as it came
  if (int rc = sample_launch(q, seed, first, centre, gen, mode, dc, dg)) return rc;
  if (mem == TZ_MEM_HOST) TZ_HIP(hipMemcpy(out, dout.p, extent * sizeof(double), hipMemcpyDeviceToHost));
  else TZ_HIP(hipDeviceSynchronize());
  return TZ_OK;
}

int tz_genstack_create(int device, const tz_genstack_desc* d, tz_genstack** out) {
  if (!d || !out) TZ_FAIL(TZ_ERR_INVALID, "null argument");
  int rc = tz_genstack_plan_check(*d, g_err);
  if (rc || (rc = use_device(device))) return rc;
  TzGenstackPlan plan;
  if ((rc = tz_genstack_plan_build(*d, plan, g_err))) return rc;
  std::unique_ptr<tz_genstack> g(new tz_genstack());
  const size_t n = d->n, m = d->m, p = n + m;
  g->device = device; g->n = d->n; g->m = d->m; g->N = d->N; g->nseg = d->nseg; g->rec = plan.rec;
  g->seg_ptr.assign(d->seg_ptr, d->seg_ptr + d->nseg + 1);
  g->G = plan.G; g->nchunk = plan.nchunk; g->mfma = plan.mfma; g->rows_mf = plan.rows_mf; g->have_cZ = plan.have_cZ;
  TZ_HIP(g->recs_mf.upload(plan.mf)); TZ_HIP(g->chunks_m.upload(plan.chunks_m)); TZ_HIP(g->recs_mfn.upload(plan.mfn));
  TZ_HIP(g->recs_lit.upload(plan.lit)); TZ_HIP(g->recs_sorted.upload(plan.srt));
  TZ_HIP(g->src_lit.upload(d->src, (size_t)std::max<int64_t>(plan.G, 1)));
  TZ_HIP(g->chunks.upload(plan.chunks)); TZ_HIP(g->seg_chunk_ptr.upload(plan.seg_chunk_ptr));
  TZ_HIP(g->c0.upload(d->c0, (size_t)d->nseg * n)); TZ_HIP(g->cE.upload(d->cE, (size_t)d->nseg * n * n));
  if (plan.have_cZ) TZ_HIP(g->cZ.upload(d->cZ, (size_t)d->nseg * d->N * n * p));
  TZ_HIP(g->K.upload(d->K, m * n));
  TZ_HIP(hipEventCreate(&g->ev0)); TZ_HIP(hipEventCreate(&g->ev1));
  *out = g.release();
  return TZ_OK;
}

int tz_genstack_destroy(tz_genstack* g) {
  if (!g) return TZ_OK;
  (void)hipSetDevice(g->device);
  (void)hipDeviceSynchronize();
  if (g->ev0) (void)hipEventDestroy(g->ev0);
  if (g->ev1) (void)hipEventDestroy(g->ev1);
  delete g;
  return TZ_OK;
}

int tz_genstack_info(tz_genstack* g, int64_t* generators, int64_t* stack_bytes, int64_t* chunks) {
  if (!g) TZ_FAIL(TZ_ERR_INVALID, "null handle");
  if (generators) *generators = g->G;
  if (stack_bytes) *stack_bytes = g->G * g->rec * (int64_t)sizeof(double);
  if (chunks) *chunks = g->nchunk;
  return TZ_OK;
}

int tz_genstack_intervals(tz_genstack* g, int32_t B, const double* e0, const double* zeta,
                          double* centre, double* rad_x, double* rad_u, double* kernel_ms, int mem) {
  if (!g || !e0 || !zeta || !centre || !rad_x || !rad_u) TZ_FAIL(TZ_ERR_INVALID, "null argument");
  if (B <= 0) TZ_FAIL(TZ_ERR_INVALID, "batch size must be positive");
  TZ_HIP(hipSetDevice(g->device));
  const int n = g->n, m = g->m, p = n + m;
  const double *de0 = nullptr, *dz = nullptr;
  int rc = gs_inputs(g, B, e0, zeta, mem, &de0, &dz);
  if (rc) return rc;
  if (int rcp = gs_reserve_partial(g, B)) return rcp;
  double *dc = centre, *drx = rad_x, *dru = rad_u;
  if (mem == TZ_MEM_HOST) {
    TZ_HIP(g->o_c.alloc((size_t)B * g->nseg * n)); TZ_HIP(g->o_rx.alloc((size_t)B * g->nseg * n)); TZ_HIP(g->o_ru.alloc((size_t)B * g->nseg * m));
    dc = g->o_c.p; drx = g->o_rx.p; dru = g->o_ru.p;
  }
  int rc2 = gs_eval(g, B, de0, dz, dc, drx, dru, 0);
  if (rc2) return rc2;
  if (mem == TZ_MEM_HOST) {
    TZ_HIP(hipMemcpy(centre, dc, (size_t)B * g->nseg * n * sizeof(double), hipMemcpyDeviceToHost));
    TZ_HIP(hipMemcpy(rad_x, drx, (size_t)B * g->nseg * n * sizeof(double), hipMemcpyDeviceToHost));
    TZ_HIP(hipMemcpy(rad_u, dru, (size_t)B * g->nseg * m * sizeof(double), hipMemcpyDeviceToHost));
  }
  if (kernel_ms) {
    TZ_HIP(hipEventSynchronize(g->ev1));
    float ms = 0.f;
    TZ_HIP(hipEventElapsedTime(&ms, g->ev0, g->ev1));
    *kernel_ms = ms;
  }
  return TZ_OK;
}

int tz_problem_attach_tube_stack(tz_problem* p, tz_genstack* g) {
  if (!p) TZ_FAIL(TZ_ERR_INVALID, "null problem");
  if (g) {
    if (g->device != p->device || g->n != p->n || g->m != p->m) TZ_FAIL(TZ_ERR_INVALID, "stack and problem differ in device or dimensions");
    if (g->nseg < p->N) TZ_FAIL(TZ_ERR_INVALID, "the stack holds %d tubes, the problem needs %d", g->nseg, p->N);
    p->fuse_enabled = false;                                   // the fused step computes theta in-kernel from the collapsed recursion
  }
  p->tube_stack = g;
  return TZ_OK;
}

int tz_genstack_values(tz_genstack* g, int32_t seg, int32_t B, const double* e0, const double* zeta, double* Z, int mem) {
  if (!g || !e0 || !zeta || !Z) TZ_FAIL(TZ_ERR_INVALID, "null argument");
  if (B <= 0 || seg < 0 || seg >= g->nseg) TZ_FAIL(TZ_ERR_INVALID, "bad batch size or tube index");
  TZ_HIP(hipSetDevice(g->device));
  const int n = g->n, m = g->m, p = n + m;
  const double *de0 = nullptr, *dz = nullptr;
  int rc = gs_inputs(g, B, e0, zeta, mem, &de0, &dz);
  if (rc) return rc;
  const int ngen = g->seg_ptr[seg + 1] - g->seg_ptr[seg];
  const size_t cnt = (size_t)B * n * (1 + ngen);
  double* dZ = Z;
  if (mem == TZ_MEM_HOST) { TZ_HIP(g->o_Z.alloc(cnt)); dZ = g->o_Z.p; }
  GsValuesParams q{B, n, m, g->N, seg, ngen, g->rec, g->recs_lit.p + (size_t)g->seg_ptr[seg] * g->rec, g->src_lit.p + g->seg_ptr[seg],
                   g->c0.p + (size_t)seg * n, g->cE.p + (size_t)seg * n * n, g->have_cZ ? g->cZ.p + (size_t)seg * g->N * n * p : nullptr, de0, dz, dZ};
  const size_t total = (size_t)B * (1 + ngen);
  hipLaunchKernelGGL(tz_genstack_values_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, q);
  TZ_HIP(hipGetLastError());
  if (mem == TZ_MEM_HOST) TZ_HIP(hipMemcpy(Z, dZ, cnt * sizeof(double), hipMemcpyDeviceToHost));
  return TZ_OK;
}

int tz_problem_create(int device, const tz_problem_desc* d, tz_problem** out) {
  if (!d || !out) TZ_FAIL(TZ_ERR_INVALID, "null argument");
  int rc = tz_plan_check(*d, g_err);               // before the device query: a machine without a GPU reports a bad description as such
  if (rc || (rc = use_device(device))) return rc;
  TzPlan plan;
  if ((rc = tz_plan_build(*d, plan, g_err))) return rc;

  tz_problem* p = new tz_problem();
  std::unique_ptr<tz_problem> guard(p);
  p->device = device;
  p->n = d->n; p->m = d->m; p->N = d->N; p->nz = d->nz; p->mi = d->mi; p->ntheta = d->ntheta;
  p->npar = d->par.rows; p->nc_rows = d->nc_rows; p->pmax = d->pmax;
  p->max_iter = d->max_iter > 0 ? d->max_iter : 40;
  p->tol = d->tol > 0 ? d->tol : 1e-10; p->reg = d->reg > 0 ? d->reg : 1e-12;
  p->step_frac = (d->step_frac > 0 && d->step_frac < 1) ? d->step_frac : 0.99;
  p->cost_scale = d->cost_scale; p->r0 = d->r0;
  p->pl = plan;
  p->fuse_enabled = plan.fused; p->have_shift = !plan.shift_var.empty();
  p->ipm_fn = ipm_kernel_for(plan.maxr, plan.ncg, plan.wgs_per_cu, plan.tt);
  if (!p->ipm_fn) TZ_FAIL(TZ_ERR_UNSUPPORTED, TZ_NO_VARIANT);

  const size_t n = d->n, m = d->m, N = d->N;
  TZ_HIP(p->vpos.upload(plan.vpos));
  TZ_HIP(p->P.upload(plan.P)); TZ_HIP(p->Gp.upload(plan.Gp)); TZ_HIP(p->smask.upload(plan.smask));
  TZ_HIP(p->eg.upload(plan.eg)); TZ_HIP(p->et.upload(plan.et));
  TZ_HIP(p->klist.upload(plan.klist)); TZ_HIP(p->items.upload(plan.items)); TZ_HIP(p->item_ptr.upload(plan.item_ptr));
  TZ_HIP(p->q.upload(plan.q)); TZ_HIP(p->h.upload(plan.h)); TZ_HIP(p->par.upload(plan.par));
  TZ_HIP(p->par_lo.upload(d->par_lo, (size_t)p->npar)); TZ_HIP(p->par_hi.upload(d->par_hi, (size_t)p->npar));
  TZ_HIP(p->Dz.upload(d->Dz, (size_t)d->nz));
  TZ_HIP(p->recy.upload(plan.recy)); TZ_HIP(p->rec0.upload(plan.rec0)); TZ_HIP(p->recx.upload(plan.recx));
  TZ_HIP(p->Phi.upload(d->Phi, (N + 1) * n * n));
  TZ_HIP(p->Gam.upload(d->Gam, (N + 1) * n * N * m));
  TZ_HIP(p->r1.upload(d->r1, n)); TZ_HIP(p->R2.upload(d->R2, n * n));
  TZ_HIP(p->CK.upload(d->CK, n * n)); TZ_HIP(p->DK.upload(d->DK, n * n));
  TZ_HIP(p->K.upload(d->K, m * n));
  TZ_HIP(p->CKpow.upload(plan.CKpow)); TZ_HIP(p->Ttube.upload(plan.Ttube));
  TZ_HIP(p->power.upload(d->power, N));
  TZ_HIP(p->row_of.upload(plan.row_of)); TZ_HIP(p->act_scale.upload(plan.act_scale));
  TZ_HIP(p->shift_var.upload(plan.shift_var)); TZ_HIP(p->shift_row.upload(plan.shift_row));
  TZ_HIP(p->shift_xs.upload(plan.shift_xs)); TZ_HIP(p->shift_ls.upload(plan.shift_ls));
  TZ_HIP(p->gunits.upload(plan.gunits)); TZ_HIP(p->gunit_ptr.upload(plan.gunit_ptr));
  p->permc = std::move(plan.permc); p->permr = std::move(plan.permr);      // tz_debug_fetch; the other host tables end here

  TZ_HIP(hipFuncSetAttribute((const void*)p->ipm_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->pl.lds_bytes));
  if (p->prof) { TZ_HIP(p->prof_buf.alloc(PH_COUNT + 16)); TZ_HIP(hipMemset(p->prof_buf.p, 0, (PH_COUNT + 16) * sizeof(unsigned long long))); }
  TZ_HIP(p->work_buf.alloc(3));
  TZ_HIP(hipMemset(p->work_buf.p, 0, 3 * sizeof(unsigned long long)));
  TZ_HIP(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
  p->own_stream = true;
  *out = guard.release();
  return TZ_OK;
}

int tz_problem_destroy(tz_problem* p) {
  if (!p) return TZ_OK;
  (void)hipSetDevice(p->device);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  for (int k = 0; k < K_COUNT; ++k)
    for (auto& e : p->ev_pool[k]) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  if (p->own_stream && p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
  return TZ_OK;
}

int tz_problem_set_stream(tz_problem* p, void* stream) {
  if (!p) TZ_FAIL(TZ_ERR_INVALID, "null problem");
  TZ_HIP(hipSetDevice(p->device));
  if (p->stream) TZ_HIP(hipStreamSynchronize(p->stream));
  if (p->own_stream && p->stream) { TZ_HIP(hipStreamDestroy(p->stream)); p->own_stream = false; }
  if (stream == nullptr) { TZ_HIP(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking)); p->own_stream = true; }
  else p->stream = (hipStream_t)stream;
  return TZ_OK;
}

int tz_problem_sync(tz_problem* p) {
  if (!p) TZ_FAIL(TZ_ERR_INVALID, "null problem");
  TZ_HIP(hipSetDevice(p->device));
  TZ_HIP(hipStreamSynchronize(p->stream));
  return TZ_OK;
}

int tz_solve_batch(tz_problem* p, int32_t B, const double* xbar0, const double* e0, double* v, double* xbar,
                   double* cost, int32_t* status, int32_t* iters, uint8_t* active, int mem) {
  if (!p || !xbar0 || !e0 || !v || !xbar || !cost || !status) TZ_FAIL(TZ_ERR_INVALID, "null argument");
  if (B < 0) TZ_FAIL(TZ_ERR_INVALID, "negative batch size");
  if (B == 0) return TZ_OK;
  TZ_HIP(hipSetDevice(p->device));
  int rc = ensure_workspace(p, B);
  if (rc) return rc;
  p->warm.invalidate();
  const size_t bn = (size_t)B * p->n * sizeof(double);
  if (mem == TZ_MEM_DEVICE) {
    return launch_solve(p, B, xbar0, e0, v, xbar, cost, status, iters, active);
  }
  if (mem != TZ_MEM_HOST) TZ_FAIL(TZ_ERR_INVALID, "mem must be TZ_MEM_HOST or TZ_MEM_DEVICE");
  hipStream_t st = p->stream;
  TZ_HIP(hipMemcpyAsync(p->in_x0.p, xbar0, bn, hipMemcpyHostToDevice, st));
  TZ_HIP(hipMemcpyAsync(p->in_e0.p, e0, bn, hipMemcpyHostToDevice, st));
  rc = launch_solve(p, B, p->in_x0.p, p->in_e0.p, p->v.p, p->xbar.p, p->cost.p, p->status.p, p->iters.p, active ? p->active.p : nullptr);
  if (rc) return rc;
  TZ_HIP(hipMemcpyAsync(v, p->v.p, (size_t)B * p->N * p->m * sizeof(double), hipMemcpyDeviceToHost, st));
  TZ_HIP(hipMemcpyAsync(xbar, p->xbar.p, (size_t)B * (p->N + 1) * p->n * sizeof(double), hipMemcpyDeviceToHost, st));
  TZ_HIP(hipMemcpyAsync(cost, p->cost.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
  TZ_HIP(hipMemcpyAsync(status, p->status.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
  if (iters) TZ_HIP(hipMemcpyAsync(iters, p->iters.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
  if (active) TZ_HIP(hipMemcpyAsync(active, p->active.p, (size_t)B * p->nc_rows, hipMemcpyDeviceToHost, st));
  TZ_HIP(hipStreamSynchronize(st));
  return TZ_OK;
}

int tz_problem_store_start(tz_problem* p, const double* xbar0, const double* e0) {
  if (!p) TZ_FAIL(TZ_ERR_INVALID, "null problem");
  if (!xbar0 || !e0) { p->warm.set_ref(false); return TZ_OK; }                       // NULL: forget the stored start
  TZ_HIP(hipSetDevice(p->device));
  int rc = ensure_workspace(p, 1);
  if (rc) return rc;
  TZ_HIP(hipMemcpyAsync(p->in_x0.p, xbar0, (size_t)p->n * sizeof(double), hipMemcpyHostToDevice, p->stream));
  TZ_HIP(hipMemcpyAsync(p->in_e0.p, e0, (size_t)p->n * sizeof(double), hipMemcpyHostToDevice, p->stream));
  rc = launch_solve(p, 1, p->in_x0.p, p->in_e0.p, p->v.p, p->xbar.p, p->cost.p, p->status.p, p->iters.p, nullptr);
  if (rc) return rc;
  int st = -1;
  TZ_HIP(hipMemcpyAsync(&st, p->status.p, sizeof(int), hipMemcpyDeviceToHost, p->stream));
  TZ_HIP(hipStreamSynchronize(p->stream));
  if (st != 0) TZ_FAIL(TZ_ERR_INVALID, "the reference point is not solvable (status %d): no start stored", st);
  TZ_HIP(p->warm.ref_x.alloc((size_t)p->nz)); TZ_HIP(p->warm.ref_lam.alloc((size_t)p->mi));
  TZ_HIP(hipMemcpyAsync(p->warm.ref_x.p, p->x.p, (size_t)p->nz * sizeof(double), hipMemcpyDeviceToDevice, p->stream));
  TZ_HIP(hipMemcpyAsync(p->warm.ref_lam.p, p->lam.p, (size_t)p->mi * sizeof(double), hipMemcpyDeviceToDevice, p->stream));
  TZ_HIP(hipStreamSynchronize(p->stream));
  p->warm.set_ref(true);
  return TZ_OK;
}

// The closed-loop entry points and their *_plants forms (per_traj: A_true is B x n x n, B_true B x n x m) differ in the plant strides only.
static void set_plant(const tz_problem* p, ClosedLoopIO& io, const double* A, const double* Bm, bool per_traj) {
  io.A = A; io.Bm = Bm;
  io.A_stride = per_traj ? (size_t)p->n * p->n : 0; io.B_stride = per_traj ? (size_t)p->n * p->m : 0;
}

static int mpc_step(tz_problem* p, int32_t B, double* x, double* xbar, double* e, const double* w,
                    const double* A_true, const double* B_true, bool per_traj, double* u_out, double* cost, int32_t* status) {
  if (!p || !x || !xbar || !e || !w || !A_true || !B_true || !cost || !status) TZ_FAIL(TZ_ERR_INVALID, "null argument");
  if (B <= 0) TZ_FAIL(TZ_ERR_INVALID, "batch size must be positive");
  TZ_HIP(hipSetDevice(p->device));
  if (int rc = ensure_workspace(p, B)) return rc;
  ClosedLoopIO io{};
  io.x = x; io.xbar = xbar; io.e = e; io.w = w; io.w_stride = (size_t)p->n; set_plant(p, io, A_true, B_true, per_traj);
  io.u_out = u_out; io.u_stride = (size_t)p->m; io.cost = cost; io.cost_stride = 1;
  io.status = status;                       // the solver status itself; no sticky record
  return run_closed_loop(p, B, 1, io);
}

static int mpc_run(tz_problem* p, int32_t B, int32_t K, double* x, double* xbar, double* e, const double* w,
                   const double* A_true, const double* B_true, bool per_traj, double* u_out, double* cost, int32_t* status) {
  if (!p || !x || !xbar || !e || !w || !A_true || !B_true || !cost || !status) TZ_FAIL(TZ_ERR_INVALID, "null argument");
  if (B <= 0 || K <= 0) TZ_FAIL(TZ_ERR_INVALID, "B and K must be positive");
  TZ_HIP(hipSetDevice(p->device));
  if (int rc = ensure_workspace(p, B)) return rc;
  ClosedLoopIO io{};
  io.x = x; io.xbar = xbar; io.e = e; io.w = w; io.w_stride = (size_t)p->n; io.w_step = (size_t)B * p->n; set_plant(p, io, A_true, B_true, per_traj);
  io.u_out = u_out; io.u_stride = (size_t)p->m; io.cost = cost; io.cost_stride = 1;      // u and cost of the last step survive
  io.status = p->status.p; io.sticky = status; io.sticky_fresh = true;                   // the caller sees the first failure of the run
  return run_closed_loop(p, B, K, io);
}

static int simulate_batch(tz_problem* p, int32_t B, int32_t T, const double* x0, const double* noise,
                          const double* A_true, const double* B_true, bool per_traj, double* x_traj, double* u_traj,
                          double* cost, int32_t* status, int mem) {
  if (!p || !x0 || !noise || !A_true || !B_true || !x_traj || !u_traj || !status) TZ_FAIL(TZ_ERR_INVALID, "null argument");
  if (B <= 0 || T <= 0) TZ_FAIL(TZ_ERR_INVALID, "B and T must be positive");
  TZ_HIP(hipSetDevice(p->device));
  if (int rc = ensure_workspace(p, B)) return rc;
  hipStream_t st = p->stream;
  const int n = p->n, m = p->m;
  const bool host = (mem == TZ_MEM_HOST);
  if (!host && mem != TZ_MEM_DEVICE) TZ_FAIL(TZ_ERR_INVALID, "mem must be TZ_MEM_HOST or TZ_MEM_DEVICE");
  const double *dA = A_true, *dB = B_true, *dnoise = noise;
  double *dx = x_traj, *du = u_traj, *dcost = cost;
  if (host) {
    const size_t np = per_traj ? (size_t)B : 1;
    TZ_HIP(p->plantA.upload(A_true, np * n * n)); TZ_HIP(p->plantB.upload(B_true, np * n * m));
    TZ_HIP(p->noise.upload(noise, (size_t)B * T * n));
    TZ_HIP(p->xtraj.alloc((size_t)B * (T + 1) * n)); TZ_HIP(p->utraj.alloc((size_t)B * T * m));
    TZ_HIP(p->costtraj.alloc((size_t)B * T));
    dA = p->plantA.p; dB = p->plantB.p; dnoise = p->noise.p; dx = p->xtraj.p; du = p->utraj.p; dcost = p->costtraj.p;
  } else if (!cost) {
    TZ_HIP(p->costtraj.alloc((size_t)B * T)); dcost = p->costtraj.p;
  }
  const hipMemcpyKind in = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  TZ_HIP(hipMemcpy2DAsync(dx, (size_t)(T + 1) * n * sizeof(double), x0, (size_t)n * sizeof(double), (size_t)n * sizeof(double), B, in, st));
  TZ_HIP(hipMemcpyAsync(p->st_x.p, x0, (size_t)B * n * sizeof(double), in, st));
  TZ_HIP(hipMemcpyAsync(p->st_xbar.p, p->st_x.p, (size_t)B * n * sizeof(double), hipMemcpyDeviceToDevice, st));   // xbar = x0 (:69)
  TZ_HIP(hipMemsetAsync(p->st_e.p, 0, (size_t)B * n * sizeof(double), st));                                        // e = 0   (:70)
  TZ_HIP(hipMemsetAsync(p->sticky.p, 0, (size_t)B * sizeof(int), st));
  ClosedLoopIO io{};
  io.x = p->st_x.p; io.xbar = p->st_xbar.p; io.e = p->st_e.p; set_plant(p, io, dA, dB, per_traj);
  io.w = dnoise; io.w_stride = (size_t)T * n; io.w_step = (size_t)n;
  io.u_out = du; io.u_stride = (size_t)T * m; io.u_step = (size_t)m;
  io.x_out = dx + n; io.x_stride = (size_t)(T + 1) * n; io.x_step = (size_t)n;
  io.cost = dcost; io.cost_stride = (size_t)T; io.cost_step = 1;                         // a cost per step
  io.status = p->status.p; io.sticky = p->sticky.p; io.fresh = true;                     // the stored start if there is one, else cold
  if (int rc = run_closed_loop(p, B, T, io)) return rc;
  if (host) {
    TZ_HIP(hipMemcpyAsync(x_traj, dx, (size_t)B * (T + 1) * n * sizeof(double), hipMemcpyDeviceToHost, st));
    TZ_HIP(hipMemcpyAsync(u_traj, du, (size_t)B * T * m * sizeof(double), hipMemcpyDeviceToHost, st));
    if (cost) TZ_HIP(hipMemcpyAsync(cost, dcost, (size_t)B * T * sizeof(double), hipMemcpyDeviceToHost, st));
    TZ_HIP(hipMemcpyAsync(status, p->sticky.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    TZ_HIP(hipStreamSynchronize(st));
  } else {
    TZ_HIP(hipMemcpyAsync(status, p->sticky.p, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, st));
  }
  return TZ_OK;
}

int tz_mpc_step(tz_problem* p, int32_t B, double* x, double* xbar, double* e, const double* w,
                const double* A_true, const double* B_true, double* u_out, double* cost, int32_t* status) {
  return mpc_step(p, B, x, xbar, e, w, A_true, B_true, false, u_out, cost, status);
}
int tz_mpc_step_plants(tz_problem* p, int32_t B, double* x, double* xbar, double* e, const double* w,
                       const double* A_true, const double* B_true, double* u_out, double* cost, int32_t* status) {
  return mpc_step(p, B, x, xbar, e, w, A_true, B_true, true, u_out, cost, status);
}

int tz_mpc_run(tz_problem* p, int32_t B, int32_t K, double* x, double* xbar, double* e, const double* w,
               const double* A_true, const double* B_true, double* u_out, double* cost, int32_t* status) {
  return mpc_run(p, B, K, x, xbar, e, w, A_true, B_true, false, u_out, cost, status);
}
int tz_mpc_run_plants(tz_problem* p, int32_t B, int32_t K, double* x, double* xbar, double* e, const double* w,
                      const double* A_true, const double* B_true, double* u_out, double* cost, int32_t* status) {
  return mpc_run(p, B, K, x, xbar, e, w, A_true, B_true, true, u_out, cost, status);
}

int tz_simulate_batch(tz_problem* p, int32_t B, int32_t T, const double* x0, const double* noise,
                      const double* A_true, const double* B_true, double* x_traj, double* u_traj,
                      double* cost, int32_t* status, int mem) {
  return simulate_batch(p, B, T, x0, noise, A_true, B_true, false, x_traj, u_traj, cost, status, mem);
}
int tz_simulate_batch_plants(tz_problem* p, int32_t B, int32_t T, const double* x0, const double* noise,
                             const double* A_true, const double* B_true, double* x_traj, double* u_traj,
                             double* cost, int32_t* status, int mem) {
  return simulate_batch(p, B, T, x0, noise, A_true, B_true, true, x_traj, u_traj, cost, status, mem);
}

int tz_problem_set_warm_shift(tz_problem* p, int32_t policy) {
  if (!p) TZ_FAIL(TZ_ERR_INVALID, "null problem");
  if (policy < 0) TZ_FAIL(TZ_ERR_INVALID, "policy must be >= 0");
  if (policy != 0 && !p->have_shift) TZ_FAIL(TZ_ERR_INVALID, "the problem was created without shift maps");
  p->shift_policy = policy;
  return TZ_OK;
}

int tz_problem_set_stopping(tz_problem* p, double res_factor, double mu_factor) {
  if (!p) TZ_FAIL(TZ_ERR_INVALID, "null problem");
  if (!(res_factor >= 1.0) || !(mu_factor > 0.0) || !(mu_factor <= 1.0)) TZ_FAIL(TZ_ERR_INVALID, "need res_factor >= 1 and 0 < mu_factor <= 1");
  p->res_factor = res_factor; p->mu_factor = mu_factor;
  return TZ_OK;
}

int tz_problem_set_warm_quiet(tz_problem* p, int32_t quiet_steps) {
  if (!p) TZ_FAIL(TZ_ERR_INVALID, "null problem");
  if (quiet_steps < 0) TZ_FAIL(TZ_ERR_INVALID, "quiet_steps must be >= 0");
  p->shift_quiet = quiet_steps;
  return TZ_OK;
}

int tz_problem_set_warm_push(tz_problem* p, double floor, double gain, double cap) {
  if (!p) TZ_FAIL(TZ_ERR_INVALID, "null problem");
  if (!(floor > 0.0) || !(gain >= 0.0) || !(cap >= floor)) TZ_FAIL(TZ_ERR_INVALID, "floor must be positive, gain non-negative, cap >= floor");
  p->warm_floor = floor; p->warm_gain = gain; p->warm_cap = cap;
  return TZ_OK;
}

int tz_problem_reset_warm(tz_problem* p) {
  if (!p) TZ_FAIL(TZ_ERR_INVALID, "null problem");
  p->warm.invalidate();
  if (p->Bcap > 0) {
    TZ_HIP(hipSetDevice(p->device));
    TZ_HIP(hipMemsetAsync(p->shift_state.p, 0, (size_t)p->Bcap * sizeof(int), p->stream));
  }
  return TZ_OK;
}

int tz_timing_enable(tz_problem* p, int enable) {
  if (!p) TZ_FAIL(TZ_ERR_INVALID, "null problem");
  TZ_HIP(hipSetDevice(p->device));
  if (p->timing) drain_timing(p);
  p->timing = enable != 0;
  if (p->timing)                                   // events are created here, not inside a timed region
    for (int k = 0; k < K_COUNT; ++k)
      while (p->ev_pool[k].size() < 512) {
        hipEvent_t a, b;
        TZ_HIP(hipEventCreate(&a)); TZ_HIP(hipEventCreate(&b));
        p->ev_pool[k].push_back({a, b});
      }
  TZ_HIP(hipStreamSynchronize(p->stream));
  TZ_HIP(hipMemset(p->work_buf.p, 0, 3 * sizeof(unsigned long long)));
  for (int k = 0; k < K_COUNT; ++k) { p->t_ms[k] = 0; p->t_count[k] = 0; }
  return TZ_OK;
}

int tz_timing_get(tz_problem* p, int kernel, double* total_ms, int64_t* launches) {
  if (!p || kernel < 0 || kernel >= K_COUNT || !total_ms || !launches) TZ_FAIL(TZ_ERR_INVALID, "bad argument");
  TZ_HIP(hipSetDevice(p->device));
  drain_timing(p);
  *total_ms = p->t_ms[kernel]; *launches = p->t_count[kernel];
  return TZ_OK;
}

int tz_ipm_work_get(tz_problem* p, int64_t* factorizations, int64_t* trajectory_solves, int64_t* max_factorizations_one_trajectory) {
  if (!p || !factorizations || !trajectory_solves) TZ_FAIL(TZ_ERR_INVALID, "null argument");
  TZ_HIP(hipSetDevice(p->device));
  TZ_HIP(hipStreamSynchronize(p->stream));
  unsigned long long h[3];
  TZ_HIP(hipMemcpy(h, p->work_buf.p, sizeof(h), hipMemcpyDeviceToHost));
  *factorizations = (int64_t)h[0]; *trajectory_solves = (int64_t)h[1];
  if (max_factorizations_one_trajectory) *max_factorizations_one_trajectory = (int64_t)h[2];
  return TZ_OK;
}

int tz_ipm_plan_info(tz_problem* p, int64_t* mfma_gram_per_iter, int64_t* mfma_chol_per_iter, int64_t* mfma_issued_per_iter,
                     int64_t* lds_bytes, int64_t* patch_bytes) {
  if (!p) TZ_FAIL(TZ_ERR_INVALID, "null problem");
  if (mfma_gram_per_iter) *mfma_gram_per_iter = p->pl.mfma_gram;
  if (mfma_chol_per_iter) *mfma_chol_per_iter = p->pl.mfma_chol;
  if (mfma_issued_per_iter) *mfma_issued_per_iter = p->pl.mfma_issued;
  if (lds_bytes) *lds_bytes = (int64_t)p->pl.lds_bytes;
  if (patch_bytes) *patch_bytes = (int64_t)p->Gp.n * 8;
  return TZ_OK;
}

int tz_problem_plan_get(tz_problem* p, int32_t* fused, int32_t* superstep_gram, int32_t* staircase) {
  if (!p) TZ_FAIL(TZ_ERR_INVALID, "null problem");
  if (fused) *fused = p->fuse_enabled ? 1 : 0;
  if (superstep_gram) *superstep_gram = p->pl.ksplit ? 1 : 0;
  if (staircase) *staircase = p->pl.staircase ? 1 : 0;
  return TZ_OK;
}

int tz_debug_fetch(tz_problem* p, int32_t b, int what, double* out, int32_t capacity) {
  if (!p || !out) TZ_FAIL(TZ_ERR_INVALID, "null argument");
  if (b < 0 || b >= p->lastB) TZ_FAIL(TZ_ERR_INVALID, "trajectory %d outside the last batch (%d)", b, p->lastB);
  TZ_HIP(hipSetDevice(p->device));
  TZ_HIP(hipStreamSynchronize(p->stream));
  const double* src = nullptr; int len = 0;
  switch (what) {
    case 0: src = p->theta.p + (size_t)b * p->ntheta; len = p->ntheta; break;
    case 1: src = p->qv.p + (size_t)b * p->nz; len = p->nz; break;
    case 2: src = p->hv.p + (size_t)b * p->mi; len = p->mi; break;
    case 3: src = p->x.p + (size_t)b * p->nz; len = p->nz; break;
    case 4: src = p->s.p + (size_t)b * p->mi; len = p->mi; break;
    case 5: src = p->lam.p + (size_t)b * p->mi; len = p->mi; break;
    case 6: {   // diagnostic build: per-phase cycle sums of workgroup 0 (as doubles)
      if (!p->prof) TZ_FAIL(TZ_ERR_INVALID, "per-phase clocks exist only in the diagnostic build of the library (libtzddpc_hip_prof.so)");
      unsigned long long h[PH_COUNT + 16];
      TZ_HIP(hipMemcpy(h, p->prof_buf.p, sizeof(h), hipMemcpyDeviceToHost));
      if (capacity < PH_COUNT + 16) TZ_FAIL(TZ_ERR_INVALID, "capacity too small");
      for (int i = 0; i < PH_COUNT + 16; ++i) out[i] = (double)h[i];
      TZ_HIP(hipMemset(p->prof_buf.p + 32, 0, 6 * sizeof(unsigned long long)));      // slots 32..37: sums of other waves (atomics), restart
      return PH_COUNT + 16;
    }
    case 7: {   // interior-point iterations of every trajectory of the last launch (b ignored)
      if (capacity < p->lastB) TZ_FAIL(TZ_ERR_INVALID, "capacity %d < %d", capacity, p->lastB);
      std::vector<int> h((size_t)p->lastB);
      TZ_HIP(hipMemcpy(h.data(), p->iters.p, h.size() * sizeof(int), hipMemcpyDeviceToHost));
      for (int i = 0; i < p->lastB; ++i) out[i] = (double)h[i];
      return p->lastB;
    }
    default: TZ_FAIL(TZ_ERR_INVALID, "unknown debug item %d", what);
  }
  if (capacity < len) TZ_FAIL(TZ_ERR_INVALID, "capacity %d < %d", capacity, len);
  TZ_HIP(hipMemcpy(out, src, (size_t)len * sizeof(double), hipMemcpyDeviceToHost));
  const std::vector<int>* perm = (what == 1 || what == 3) ? &p->permc : ((what == 2 || what == 4 || what == 5) ? &p->permr : nullptr);
  if (perm && !perm->empty()) {                       // device order -> the caller's order
    std::vector<double> tmp(out, out + len);
    for (int i = 0; i < len; ++i) out[(*perm)[i]] = tmp[i];
  }
  return len;
}

}  // extern "C"
