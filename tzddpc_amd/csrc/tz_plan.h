// Host-side planning of the TZDDPC hot path: everything tz_problem_create / tz_genstack_create derive from a description before
// anything is uploaded -- the order of variables and rows, the padded copies and tables the kernels walk, the kernel class and its
// LDS placement.  Plain C++ (no HIP): tzddpc_hip.hip builds a plan and uploads its tables as they are; tests/test_host_plan.py
// builds the same plans on a CPU under UBSan and the libstdc++ assertions and checks every table against numpy.
#pragma once
#include "tz_layout.h"
#include "../../include/tzddpc.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

// leave the calling function with `code` and a formatted message in `err`
#define TZ_FAIL_TO(err, code, ...) do { char _b[512]; snprintf(_b, sizeof(_b), __VA_ARGS__); (err) = _b; return (code); } while (0)

typedef std::vector<std::vector<std::pair<int, double>>> TzOuts;      // per output of a sparse product: its (input index, value) pairs

// Host copy of a balanced lane-ELL table (TzEll in tz_ipm.hip.h): 16-byte records, or values and 16-bit indices (compact).
struct TzEllTable {
  int L = 1, VL = 0;
  std::vector<TzEllEnt> ent; std::vector<int> seg; std::vector<double> val; std::vector<unsigned short> idx;
};
// Host copy of a tz_affmap (CSR in the ABI) re-laid out as ELL, see TzCsr in tz_kernels.hip.h.
struct TzMapTable {
  int rows = 0, W = 1;
  std::vector<TzEllEnt> ent; std::vector<double> c0;
};

// The plan's sizes and decisions: what the library keeps for the lifetime of a problem.
struct TzPlanSizes {
  int nzp = 0, mip = 0, Tz = 0, Kc = 0, nquads = 0, nklist = 0, nP = 0;
  int maxr = 1, ncg = 1;       // rows per thread, 64-column groups: with wgs_per_cu they select the kernel variant
  bool tt = false;             // tile-triangle layout / blocked Gram / two-phase Cholesky (nz > 64 or more than 1024 rows)
  bool staircase = false;      // tile-triangle class: variables in time order, rows by last non-zero column (library-internal)
  bool ksplit = false;         // Gram by k-split (Tz <= TZ_KS_TZ; TZ_PLAN_ITEM_GRAM keeps the item plan)
  int TS = 16, ntile = 0, gu = 0;
  size_t hsize = 0;            // doubles of factor storage in LDS
  int nell = 0, ntube = 0;
  size_t lds_bytes = 0;
  int wgs_per_cu = 1;
  bool lean_epilogue = false;  // FuseParams::lean_epilogue
  bool fused = true;           // closed-loop steps in one launch (TZ_PLAN_UNFUSED: four kernels per step, same arithmetic)
  int64_t mfma_gram = 0, mfma_chol = 0, mfma_issued = 0;
};

// ... and the tables, each in the element order the kernels read.
struct TzPlan : TzPlanSizes {
  std::vector<int> permc, permr;   // device variable / row i is the caller's permc[i] / permr[i]
  std::vector<int> vpos;           // staircase ordering: device position of v[k, j]; empty = identity
  std::vector<double> P, Gp;
  std::vector<int> klist, item_ptr, smask;                             // these three and items: quad class only
  std::vector<IpmItem> items;
  TzEllTable eg, et;               // G x (outputs = rows) and G'v (outputs = columns)
  TzMapTable q, h, par;
  std::vector<double> CKpow, Ttube, act_scale, rec0, recx, recy;      // rec*: empty without equality elimination
  std::vector<int> row_of;
  std::vector<int> shift_var, shift_row; std::vector<double> shift_xs, shift_ls;      // empty: no shift maps
  std::vector<TzGUnit> gunits; std::vector<int> gunit_ptr;             // tile-triangle class only
};

// ---- pieces of tz_plan_build, in the order it calls them ----------------------------------------------------------------------------

// The checks that need nothing but the description's sizes and index arrays.
inline int tz_plan_check(const tz_problem_desc& d, std::string& err) {
  if (d.abi_version != TZ_ABI_VERSION) TZ_FAIL_TO(err, TZ_ERR_INVALID, "abi_version %d != %d", d.abi_version, TZ_ABI_VERSION);
  if (d.pmax > TZ_PMAX) TZ_FAIL_TO(err, TZ_ERR_UNSUPPORTED, "pmax=%d > %d powers of M_K not supported by tz_tube_kernel", d.pmax, TZ_PMAX);
  if (d.n < 1 || d.n > TZ_NMAX || d.m < 1 || d.m > TZ_MMAX) TZ_FAIL_TO(err, TZ_ERR_UNSUPPORTED, "dim_x must be 1..%d and dim_u 1..%d", TZ_NMAX, TZ_MMAX);
  if (d.N < 1 || d.nz < d.N * d.m || d.mi < 1) TZ_FAIL_TO(err, TZ_ERR_INVALID, "inconsistent sizes N=%d nz=%d mi=%d", d.N, d.nz, d.mi);
  if (d.nz > 256) TZ_FAIL_TO(err, TZ_ERR_UNSUPPORTED, "nz=%d > 256 decision variables not supported by tz_ipm_kernel", d.nz);
  if (d.mi > 6 * TZ_THREADS) TZ_FAIL_TO(err, TZ_ERR_UNSUPPORTED, "mi=%d > %d inequality rows not supported by tz_ipm_kernel", d.mi, 6 * TZ_THREADS);
  if (d.ntheta != 2 * d.n + d.N * (2 * d.n + d.m)) TZ_FAIL_TO(err, TZ_ERR_INVALID, "ntheta mismatch");
  if (d.q.rows != d.nz || d.h.rows != d.mi) TZ_FAIL_TO(err, TZ_ERR_INVALID, "affine map row counts do not match nz / mi");
  for (int k = 0; k < d.N; ++k)
    if (d.power[k] < 0 || d.power[k] > d.pmax) TZ_FAIL_TO(err, TZ_ERR_INVALID, "power[%d]=%d outside 0..pmax", k, d.power[k]);
  for (int r = 0; r < d.mi; ++r)
    if (d.row_of[r] < 0 || d.row_of[r] >= std::max(d.nc_rows, 1)) TZ_FAIL_TO(err, TZ_ERR_INVALID, "row_of[%d] out of range", r);
  const int32_t known_flags = TZ_PLAN_UNFUSED | TZ_PLAN_ITEM_GRAM | TZ_PLAN_NO_STAIRCASE;
  if (d.plan_flags & ~known_flags) TZ_FAIL_TO(err, TZ_ERR_INVALID, "plan_flags 0x%x: unknown bits 0x%x", (unsigned)d.plan_flags, (unsigned)(d.plan_flags & ~known_flags));
  return TZ_OK;
}

// Staircase ordering (tile-triangle class): the library keeps the variables in time order (v_k next to the epigraph variables
// of step k) and the rows by their last non-zero column, so that the non-zeros of G lie under a staircase: super-step s (16
// rows) touches only the tile columns 0 .. cmax[s], non-decreasing in s.  A unit of the blocked Gram is then active on a
// contiguous range of super-steps [s0, S) and runs there without a single mask test.  Purely structural: the time of v[k, j]
// (the first N m variables, reference tzddpc/tzddpc.py:155) is k, the time of any other variable the smallest, over the rows
// it appears in, of the latest input in that row.  Callers never see the ordering (outputs go through vpos / row_of).
inline void tz_plan_order(const tz_problem_desc& d, std::vector<int>& permc, std::vector<int>& permr, std::vector<int>& vpos) {
  const int nz = d.nz, mi = d.mi, nv = d.N * d.m;
  std::vector<int> rowt((size_t)mi, -1), colt((size_t)nz, 1 << 30), invc((size_t)nz);
  for (int r = 0; r < mi; ++r) for (int c = 0; c < nv; ++c) if (d.G[(size_t)r * nz + c] != 0.0) rowt[r] = std::max(rowt[r], c / d.m);
  for (int c = 0; c < nv; ++c) colt[c] = c / d.m;
  for (int c = nv; c < nz; ++c) { for (int r = 0; r < mi; ++r) if (d.G[(size_t)r * nz + c] != 0.0) colt[c] = std::min(colt[c], rowt[r]); if (colt[c] == (1 << 30)) colt[c] = d.N; }
  std::stable_sort(permc.begin(), permc.end(), [&](int a, int b) { return colt[a] < colt[b]; });
  for (int i = 0; i < nz; ++i) invc[permc[i]] = i;
  std::vector<int> last((size_t)mi, -1);
  for (int r = 0; r < mi; ++r) for (int c = 0; c < nz; ++c) if (d.G[(size_t)r * nz + c] != 0.0) last[r] = std::max(last[r], invc[c]);
  std::stable_sort(permr.begin(), permr.end(), [&](int a, int b) { return last[a] < last[b]; });
  vpos.resize((size_t)nv);
  for (int c = 0; c < nv; ++c) vpos[c] = invc[c];
}

// Longest-processing-time assignment of jobs to the TZ_NWAVES waves: by decreasing cost to the least loaded wave.  Returns the
// job indices wave by wave; span (may be null): the largest load.
inline std::vector<std::vector<int>> tz_plan_lpt(const std::vector<double>& cost, double* span = nullptr) {
  std::vector<int> order(cost.size());
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
  std::vector<std::vector<int>> per_wave(TZ_NWAVES);
  double load[TZ_NWAVES] = {0, 0, 0, 0};
  for (int idx : order) {
    int w = (int)(std::min_element(load, load + TZ_NWAVES) - load);
    per_wave[w].push_back(idx); load[w] += cost[idx];
  }
  if (span) *span = *std::max_element(load, load + TZ_NWAVES);
  return per_wave;
}

// Gram plan of the quad class: item = (block of 4 tile rows I0..I0+3, quads q0..q0+nq-1), k-list = chunks where the 16 columns
// are non-zero; the items are dealt to the waves by LPT.  G: the padded device-order copy (mip x nzp).
inline void tz_plan_items(const std::vector<double>& G, int nz, int mi, TzPlan& pl) {
  const int Tz = pl.Tz, Kc = pl.Kc, nzp = pl.nzp;
  std::vector<IpmItem> items;
  std::vector<double> cost;
  const int NB = (Tz + 3) / 4;
  for (int IB = 0; IB < NB; ++IB) {
    const int kptr = (int)pl.klist.size();
    for (int kc = 0; kc < Kc; ++kc) {
      bool nzr = false;
      for (int r = 4 * kc; r < std::min(4 * kc + 4, mi) && !nzr; ++r)
        for (int c = 16 * IB; c < std::min(16 * IB + 16, nz); ++c)
          if (G[(size_t)r * nzp + c] != 0.0) { nzr = true; break; }
      if (nzr) pl.klist.push_back(kc);
    }
    const int klen = (int)pl.klist.size() - kptr;
    for (int z = 0; z < 8; ++z) pl.klist.push_back(Kc);     // prefetch padding: the all-zero patch row
    const int Ilast = std::min(4 * IB + 3, Tz - 1);
    const int qmax = Ilast >> 2;          // quads 0..qmax exist for the last row of the block
    for (int q0 = 0; q0 <= qmax; q0 += 2) {
      IpmItem it{4 * IB, q0, std::min(2, qmax - q0 + 1), kptr, klen};
      items.push_back(it);
      cost.push_back((double)klen * 4 * it.nq + 8);
    }
  }
  const std::vector<std::vector<int>> per_wave = tz_plan_lpt(cost);
  pl.item_ptr.assign(TZ_NWAVES + 1, 0);
  pl.mfma_gram = 0;
  for (int w = 0; w < TZ_NWAVES; ++w) {
    for (int idx : per_wave[w]) {
      const IpmItem& it = items[idx];
      pl.items.push_back(it);
      const int validI = std::min(4, Tz - it.I0);
      pl.mfma_gram += (int64_t)it.klen * validI * it.nq;
      pl.mfma_issued += (int64_t)it.klen * 8;
    }
    pl.item_ptr[w + 1] = (int)pl.items.size();
  }
  pl.mfma_chol = 0;
  for (int pp = 0; pp < Tz; ++pp)
    for (int I = pp + 1; I < Tz; ++I) pl.mfma_chol += (I >> 2) - ((pp + 1) >> 2) + 1;
  pl.mfma_issued += pl.mfma_chol;
  if (pl.klist.empty()) pl.klist.push_back(0);
  pl.nklist = std::max((int)pl.klist.size(), (Kc + 3) / 4 + 1);     // the LDS k-list area doubles as the super-step mask table (ksplit)
}

// Balanced lane-ELL of a sparse matrix for the matrix-vector products of tz_ipm_kernel (TzEll in tz_ipm.hip.h).
// outs[o] = (index, value) pairs of output o; NL physical lanes per pass; the virtual lane count VL is a multiple of NL.
// compact: 8-byte values and 16-bit indices in two arrays (the tile-triangle class, see TzEll) instead of 16-byte records.
inline TzEllTable tz_plan_ell(const TzOuts& outs, int NL, int VLwant, bool compact) {
  TzEllTable t;
  int& L = t.L;
  const int VL = t.VL = ((std::max(VLwant, 1) + NL - 1) / NL) * NL;
  size_t longest = 1;
  for (auto& o : outs) longest = std::max(longest, o.size());
  for (L = 1; L <= (int)longest; ++L) {
    size_t lanes = 0;
    for (auto& o : outs) lanes += (o.size() + L - 1) / L;
    if (lanes <= (size_t)VL) break;
  }
  t.ent.assign(compact ? 0 : (size_t)VL * L, TzEllEnt{0.0, 0u, 0u});
  t.val.assign(compact ? (size_t)VL * L : 0, 0.0);
  t.idx.assign(compact ? (size_t)VL * L : 0, (unsigned short)0);
  t.seg.assign(std::max<size_t>(outs.size(), 1), 0);
  int lane = 0;
  for (size_t o = 0; o < outs.size(); ++o) {
    const int cnt = (int)((outs[o].size() + L - 1) / L);
    t.seg[o] = lane | (cnt << 16);
    for (size_t e = 0; e < outs[o].size(); ++e) {
      const int vl = lane + (int)(e / L), slot = (int)(e % L);
      const size_t pos = ((size_t)(vl / NL) * L + slot) * NL + (vl % NL);
      if (compact) { t.val[pos] = outs[o][e].second; t.idx[pos] = (unsigned short)outs[o][e].first; }
      else t.ent[pos] = TzEllEnt{outs[o][e].second, (unsigned)outs[o][e].first * 8u, 0u};
    }
    lane += cnt;
  }
  return t;
}

// ELL copy of an affine map; perm (may be null): device row i is row perm[i] of the map
inline TzMapTable tz_plan_map(const tz_affmap& m, const int* perm = nullptr) {
  TzMapTable t;
  const int rows = t.rows = m.rows;
  for (int r = 0; r < m.rows; ++r) t.W = std::max(t.W, m.ptr[r + 1] - m.ptr[r]);
  t.ent.assign((size_t)t.W * std::max(rows, 1), TzEllEnt{0.0, 0u, 0u});
  t.c0.assign((size_t)rows, 0.0);
  for (int i = 0; i < m.rows; ++i) {
    const int r = perm ? perm[i] : i;
    t.c0[i] = m.c0[r];
    for (int e = m.ptr[r]; e < m.ptr[r + 1]; ++e) t.ent[(size_t)(e - m.ptr[r]) * rows + i] = TzEllEnt{m.val[e], (unsigned)m.col[e] * 8u, 0u};
  }
  return t;
}

// Resolvent of the tube recursion (tz_kernels.hip.h, TubeParams): with X_j = |C_K^j|, U_j = |K C_K^j|,
//   R_0 = D_K, R_d = D_K Tx_{d-1};  Tx_d = sum_{j<=d} X_{d-j} R_j;  Tu_d = sum_{j<=d} U_{d-j} R_j;  and C_K^l.
inline void tz_plan_tube(const tz_problem_desc& d, std::vector<double>& ckp, std::vector<double>& T) {
  const int n = d.n, m = d.m, pm = d.pmax, nm = n + m;
  ckp.assign((size_t)(pm + 1) * n * n, 0.0); T.assign((size_t)std::max(pm, 1) * nm * n, 0.0);
  std::vector<double> R((size_t)std::max(pm, 1) * n * n, 0.0);
  auto add_product = [n](double* out, const double* A, int rows, const double* B) {      // out (rows x n) += A (rows x n) B (n x n)
    for (int i = 0; i < rows; ++i) for (int j = 0; j < n; ++j) {
      double a = 0.0;
      for (int k = 0; k < n; ++k) a += A[i * n + k] * B[k * n + j];
      out[i * n + j] += a;
    }
  };
  for (int i = 0; i < n; ++i) ckp[(size_t)i * n + i] = 1.0;
  for (int l = 1; l <= pm; ++l) add_product(&ckp[(size_t)l * n * n], d.CK, n, &ckp[(size_t)(l - 1) * n * n]);
  for (int dd = 0; dd < pm; ++dd) {
    double* Rd = &R[(size_t)dd * n * n];
    if (dd == 0) for (int e = 0; e < n * n; ++e) Rd[e] = d.DK[e];
    else add_product(Rd, d.DK, n, &T[(size_t)(dd - 1) * nm * n]);      // Tx_{d-1} = first n rows
    double* Td = &T[(size_t)dd * nm * n];
    for (int jj = 0; jj <= dd; ++jj) {
      add_product(Td, d.absCKpow + (size_t)(dd - jj) * n * n, n, &R[(size_t)jj * n * n]);
      add_product(Td + n * n, d.absKCKpow + (size_t)(dd - jj) * m * n, m, &R[(size_t)jj * n * n]);
    }
  }
}

// Tile-triangle class: tile stride, workgroups per CU and which G x table, against the LDS of a CU.  Two workgroups per CU with the
// padded tile stride if that fits, else one; the partial-sum buffer of the G x product shrinks from two virtual lanes per row to
// one (eg_small replaces pl.eg) before the tile stride loses its padding.  Returns the bytes the problem needs; more than lds_max:
// nothing fits and the plan is unchanged.
inline size_t tz_plan_place(TzPlan& pl, int ntheta, const TzEllTable& eg_small, size_t lds_max) {
  auto lds_for = [&](int TS, int nell) { return tz_ipm_lds_doubles((size_t)pl.ntile * TS, 1, pl.Tz, pl.nzp, pl.mip, pl.nklist, ntheta, 0, pl.ntube, nell) * sizeof(double); };
  const int nell_full = pl.nell, nell_small = std::max(eg_small.VL, pl.et.VL);
  struct Cand { int TS; bool small; int wgs; };
  const Cand cands[] = {{17, false, 2}, {17, true, 2}, {17, false, 1}, {17, true, 1}, {16, true, 1}};
  for (const Cand& c : cands) {
    const size_t need = lds_for(c.TS, c.small ? nell_small : nell_full);
    if (need * c.wgs <= lds_max) {
      pl.TS = c.TS; pl.wgs_per_cu = c.wgs; pl.lds_bytes = need;
      if (c.small) { pl.eg = eg_small; pl.nell = nell_small; }
      return need;
    }
  }
  return lds_for(16, nell_small);
}

// Unit plan of the blocked Gram (tile-triangle class).  byrow: the row lists of G (columns ascending).  cmaxs: last non-zero tile
// column of every super-step (non-decreasing when the staircase ordering is on); sfirst[I] = first super-step that touches tile column I.
// units: the tile index range (padded with all-zero tile columns up to a multiple of U) is cut into ranges of exactly U tiles;
// a unit is a pair of ranges (row range >= column range).  Cost = MFMAs + loads it issues; LPT over the waves; the U in
// [UMAX - 2, UMAX] with the smallest makespan wins.  Returns that makespan (1e300: no plan).
inline double tz_plan_units(const TzOuts& byrow, int UMAX, TzPlan& pl) {
  const int Tz = pl.Tz, S = (pl.Kc + 3) / 4;
  std::vector<int> cmaxs((size_t)S, -1);
  for (size_t r = 0; r < byrow.size(); ++r) if (!byrow[r].empty()) cmaxs[r >> 4] = std::max(cmaxs[r >> 4], byrow[r].back().first >> 2);
  std::vector<int> sfirst((size_t)Tz + 1, S);
  for (int sIdx = S - 1; sIdx >= 0; --sIdx) for (int I = 0; I <= cmaxs[sIdx]; ++I) sfirst[I] = sIdx;
  double best_span = 1e300;
  for (int U = std::max(1, UMAX - 2); U <= UMAX; ++U) {
    const int nrange = (Tz + U - 1) / U;
    std::vector<TzGUnit> units; std::vector<double> cost;
    for (int a = 0; a < nrange; ++a) for (int b = 0; b <= a; ++b) {
      TzGUnit u{a * U, b * U, sfirst[a * U]};
      const double per = (a == b) ? 0.5 * U * (U + 1) + 0.4 * U : (double)U * U + 0.4 * 2 * U;   // MFMAs + loads of one super-step
      units.push_back(u); cost.push_back(per * (S - u.s0 + 3) + 60.0);   // + pipeline fill, fold / store
    }
    double span = 0.0;
    const std::vector<std::vector<int>> per_wave = tz_plan_lpt(cost, &span);
    if (span < best_span) {
      best_span = span; pl.gu = U; pl.gunits.clear(); pl.gunit_ptr.assign(TZ_NWAVES + 1, 0);
      for (int w = 0; w < TZ_NWAVES; ++w) { for (int idx : per_wave[w]) pl.gunits.push_back(units[idx]); pl.gunit_ptr[w + 1] = (int)pl.gunits.size(); }
    }
  }
  return best_span;
}

// The whole plan of a problem.  Returns TZ_OK or the TZ_ERR_* code tz_problem_create reports, with its message in err.
inline int tz_plan_build(const tz_problem_desc& d, TzPlan& pl, std::string& err) {
  if (int rc = tz_plan_check(d, err)) return rc;
  pl = TzPlan();
  const int nz = d.nz, mi = d.mi, nv = d.N * d.m;
  const int Tz = pl.Tz = (nz + 3) / 4, nzp = pl.nzp = 4 * Tz;
  const int Kc = pl.Kc = (mi + 3) / 4, mip = pl.mip = 4 * Kc;
  for (int I = 0; I < Tz; ++I) pl.nquads += (I >> 2) + 1;
  pl.maxr = (mi + TZ_THREADS - 1) / TZ_THREADS; pl.ncg = (nzp + 63) / 64;
  pl.tt = (pl.ncg >= 2 || pl.maxr > 4);

  std::vector<int>& permc = pl.permc; std::vector<int>& permr = pl.permr;
  permc.resize((size_t)nz); permr.resize((size_t)mi);
  std::iota(permc.begin(), permc.end(), 0); std::iota(permr.begin(), permr.end(), 0);
  if (pl.tt && !(d.plan_flags & TZ_PLAN_NO_STAIRCASE)) { tz_plan_order(d, permc, permr, pl.vpos); pl.staircase = true; }
  std::vector<int> invc((size_t)nz), invr((size_t)mi);
  for (int i = 0; i < nz; ++i) invc[permc[i]] = i;
  for (int i = 0; i < mi; ++i) invr[permr[i]] = i;

  // padded dense copies (device order); G itself stays on the host, the kernels read its patches and the two ELL tables
  std::vector<double> G((size_t)mip * nzp, 0.0);
  pl.P.assign((size_t)nzp * nzp, 0.0); pl.Gp.assign((size_t)(Kc + 1) * (Tz + 1) * 16, 0.0);   // tile Tz of every row and the last patch row stay zero (masked operands / prefetch padding)
  for (int r = 0; r < nz; ++r) for (int c = 0; c < nz; ++c) pl.P[(size_t)r * nzp + c] = d.P[(size_t)permc[r] * nz + permc[c]];
  TzOuts byrow((size_t)mi), bycol((size_t)nz);
  for (int r = 0; r < mi; ++r) for (int c = 0; c < nz; ++c) {
    const double v = d.G[(size_t)permr[r] * nz + permc[c]];
    G[(size_t)r * nzp + c] = v;
    pl.Gp[((size_t)(r >> 2) * (Tz + 1) + (c >> 2)) * 16 + 4 * (r & 3) + (c & 3)] = v;
    if (v != 0.0) { byrow[r].push_back({c, v}); bycol[c].push_back({r, v}); }
  }
  for (int r = 0; r < nz; ++r) for (int c = 0; c < nz; ++c) if (pl.P[(size_t)r * nzp + c] != 0.0) pl.nP = r + 1;

  if (!pl.tt) {                       // quad class only: the tile-triangle Gram works from the units below and reads none of these tables
    tz_plan_items(G, nz, mi, pl);
    pl.smask.assign((size_t)(Kc + 3) / 4 + 1, 0);
    if (Tz <= 31) for (int r = 0; r < mi; ++r) for (int c = 0; c < nz; ++c) if (G[(size_t)r * nzp + c] != 0.0) pl.smask[r >> 4] |= 1 << (c >> 2);
  }
  // G x: twice as many virtual lanes as rows, so the long rows can be cut up;  G'v: the 192 lanes of waves 1-3 per pass
  pl.eg = tz_plan_ell(byrow, TZ_THREADS, 2 * mi, pl.tt);
  pl.et = tz_plan_ell(bycol, TZ_THREADS - 64, std::max(TZ_THREADS - 64, 2 * nz), pl.tt);
  pl.nell = std::max(pl.eg.VL, pl.et.VL);
  pl.q = tz_plan_map(d.q, permc.data()); pl.h = tz_plan_map(d.h, permr.data()); pl.par = tz_plan_map(d.par);

  const bool have_rec = d.rec_y || d.rec_c0 || d.rec_x0;
  if (have_rec) {                                                        // equality-eliminated problem: affine recovery of v
    if (!(d.rec_y && d.rec_c0 && d.rec_x0)) TZ_FAIL_TO(err, TZ_ERR_INVALID, "rec_c0, rec_x0 and rec_y go together");
    pl.recy.resize((size_t)nv * nz);
    for (int c = 0; c < nv; ++c) for (int k = 0; k < nz; ++k) pl.recy[(size_t)c * nz + k] = d.rec_y[(size_t)c * nz + permc[k]];
    pl.rec0.assign(d.rec_c0, d.rec_c0 + nv); pl.recx.assign(d.rec_x0, d.rec_x0 + (size_t)nv * d.n);
  }
  // xbar[1] = Phi_1 xbar0 + Gam_1 v with Gam_1 confined to v[0] (it is A xbar0 + B v[0], reference :166-170)
  pl.lean_epilogue = !have_rec;
  for (int i = 0; i < d.n && pl.lean_epilogue; ++i) for (int c = d.m; c < nv; ++c) if (d.Gam[((size_t)d.n + i) * nv + c] != 0.0) { pl.lean_epilogue = false; break; }
  tz_plan_tube(d, pl.CKpow, pl.Ttube);
  pl.row_of.resize((size_t)mi); pl.act_scale.resize((size_t)mi);
  for (int i = 0; i < mi; ++i) { pl.row_of[i] = d.row_of[permr[i]]; pl.act_scale[i] = d.act_scale[permr[i]]; }
  if (d.shift_var && d.shift_row && d.shift_xscale && d.shift_lscale) {
    for (int c = 0; c < nz; ++c) if (d.shift_var[c] < 0 || d.shift_var[c] >= nz) TZ_FAIL_TO(err, TZ_ERR_INVALID, "shift_var[%d] out of range", c);
    for (int r = 0; r < mi; ++r) if (d.shift_row[r] < 0 || d.shift_row[r] >= mi) TZ_FAIL_TO(err, TZ_ERR_INVALID, "shift_row[%d] out of range", r);
    pl.shift_var.resize((size_t)nz); pl.shift_row.resize((size_t)mi); pl.shift_xs.resize((size_t)nz); pl.shift_ls.resize((size_t)mi);
    for (int i = 0; i < nz; ++i) { pl.shift_var[i] = invc[d.shift_var[permc[i]]]; pl.shift_xs[i] = d.shift_xscale[permc[i]]; }
    for (int i = 0; i < mi; ++i) { pl.shift_row[i] = invr[d.shift_row[permr[i]]]; pl.shift_ls[i] = d.shift_lscale[permr[i]]; }
  }

  pl.ntube = (d.pmax + 1) * d.n * d.n + std::max(d.pmax, 1) * (d.n + d.m) * d.n            // tube tables
             + 3 * d.n * d.n + 2 * d.n * d.m + d.n + d.n * d.N * d.m + d.N * d.m           // recovery / plant constants
             + (d.N + 1) / 2;                                                                // power[k] (ints)
  const size_t LDS_MAX = 160 * 1024;
  auto fail_lds = [&](size_t need) { TZ_FAIL_TO(err, TZ_ERR_UNSUPPORTED, "not supported: the problem needs %zu bytes of LDS per workgroup (nz=%d, mi=%d); limit is 160 KiB", need, nz, mi); };
  if (pl.tt) {
    pl.ntile = Tz * (Tz + 1) / 2;
    pl.nklist = 2;
    const size_t need = tz_plan_place(pl, d.ntheta, tz_plan_ell(byrow, TZ_THREADS, mi, pl.tt), LDS_MAX);
    if (need > LDS_MAX) return fail_lds(need);
    pl.hsize = (size_t)pl.ntile * pl.TS;
    if (pl.maxr > 4) pl.wgs_per_cu = 1;                                // those variants exist for one workgroup per CU only
    const double span = tz_plan_units(byrow, TZ_TT_GU(pl.wgs_per_cu), pl);   // unit size <= what the chosen variant's register budget holds
    if (pl.gunits.empty()) TZ_FAIL_TO(err, TZ_ERR_UNSUPPORTED, "no Gram plan for Tz=%d", Tz);
    pl.mfma_gram = (int64_t)span; pl.mfma_chol = (int64_t)Tz * Tz * Tz / 24; pl.mfma_issued = pl.mfma_gram * TZ_NWAVES + pl.mfma_chol;
  } else {
    pl.ksplit = (Tz <= TZ_KS_TZ) && !(d.plan_flags & TZ_PLAN_ITEM_GRAM);
    pl.hsize = (size_t)pl.nquads * TZ_QSTR;
    // nz <= 64: the 128-register variant, h and G x of the rows parked in LDS
    pl.lds_bytes = tz_ipm_lds_doubles(pl.hsize, 0, Tz, nzp, mip, pl.nklist, d.ntheta, pl.ksplit ? 1 : 0, pl.ntube, pl.nell, 1) * sizeof(double);
    if (pl.lds_bytes > LDS_MAX) return fail_lds(pl.lds_bytes);
    pl.wgs_per_cu = (int)(LDS_MAX / std::max<size_t>(pl.lds_bytes, 1));
  }
  // the tube pass of the fused step keeps |C_K^l e0| (pmax n doubles) in the factor storage, which is free at that point: a short-horizon,
  // large-n problem whose factor is smaller than that runs the four-kernel step instead (tz_tube_kernel has its own scratch)
  pl.fused = !(d.plan_flags & TZ_PLAN_UNFUSED) && !((size_t)std::max(d.pmax, 1) * d.n > pl.hsize);
  return TZ_OK;
}

// ---- generator stack (K1g, tz_genstack.hip.h) ---------------------------------------------------------------------------------------

struct TzGenstackPlan {
  int rec = 0, nchunk = 0;
  int64_t G = 0;
  bool mfma = false;                        // matrix-core layout (dimensions with a compiled instance)
  int rows_mf = 0;                          // rows per generator in mf: n + m (K rows appended); mfn holds the n-row copy when rows_mf == n
  bool have_cZ = false;
  std::vector<double> lit, srt;             // records [m0 | M]: literal order (tz_genstack_values), sorted by (tube, source) (tz_genstack_intervals)
  std::vector<GsChunk> chunks; std::vector<int> seg_chunk_ptr;
  std::vector<double> mf, mfn; std::vector<GsChunkM> chunks_m;
};

inline int tz_genstack_plan_check(const tz_genstack_desc& d, std::string& err) {
  if (!d.seg_ptr || !d.src || !d.m0 || !d.M || !d.c0 || !d.cE || !d.K) TZ_FAIL_TO(err, TZ_ERR_INVALID, "null argument");
  if (d.n < 1 || d.n > TZ_NMAX || d.m < 1 || d.m > TZ_MMAX) TZ_FAIL_TO(err, TZ_ERR_UNSUPPORTED, "dim_x must be 1..%d and dim_u 1..%d", TZ_NMAX, TZ_MMAX);
  if (d.N < 1 || d.nseg < 1) TZ_FAIL_TO(err, TZ_ERR_INVALID, "N and nseg must be positive");
  return TZ_OK;
}

// Matrix-core layout of the sorted stack: per group of 4 generators (a chunk is padded with zero generators)
// [component c < RW][generator i < 4][inner k < P] of Mext = [M; K M], then [c][i] of m0ext = [m0; K m0].  RW = P: the K rows are
// appended; RW = n: only the rows [m0 | M].  cm (may be null) receives the chunk table: group offsets are the same for both RW.
inline std::vector<double> tz_genstack_plan_layout(const tz_genstack_desc& d, const TzGenstackPlan& g, int RW, std::vector<GsChunkM>* cm) {
  const int n = d.n, p = n + d.m, GD = 4 * RW * (p + 1);
  std::vector<double> mf, ext((size_t)p * (p + 1));
  for (const GsChunk& ch : g.chunks) {
    const int ng = ch.g1 - ch.g0, nq = (ng + 3) / 4;
    const size_t q0 = mf.size() / GD;
    mf.resize(mf.size() + (size_t)nq * GD, 0.0);
    for (int gi = 0; gi < ng; ++gi) {
      const double* r = &g.srt[(size_t)(ch.g0 + gi) * g.rec];            // [m0 (n) | M (n x p)]
      for (int c = 0; c < RW; ++c) {
        double m0e = 0.0;
        if (c < n) m0e = r[c]; else for (int i = 0; i < n; ++i) m0e += d.K[(size_t)(c - n) * n + i] * r[i];
        ext[(size_t)c * (p + 1)] = m0e;
        for (int k = 0; k < p; ++k) {
          double v = 0.0;
          if (c < n) v = r[n + c * p + k]; else for (int i = 0; i < n; ++i) v += d.K[(size_t)(c - n) * n + i] * r[n + i * p + k];
          ext[(size_t)c * (p + 1) + 1 + k] = v;
        }
      }
      double* gb = &mf[(q0 + gi / 4) * GD];
      const int i4 = gi & 3;
      for (int c = 0; c < RW; ++c) {
        for (int k = 0; k < p; ++k) gb[c * 4 * p + i4 * p + k] = ext[(size_t)c * (p + 1) + 1 + k];
        gb[4 * RW * p + 4 * c + i4] = ext[(size_t)c * (p + 1)];
      }
    }
    if (cm) cm->push_back(GsChunkM{ch.seg, ch.src, (int)q0, nq});
  }
  return mf;
}

inline int tz_genstack_plan_build(const tz_genstack_desc& d, TzGenstackPlan& g, std::string& err) {
  if (int rc = tz_genstack_plan_check(d, err)) return rc;
  g = TzGenstackPlan();
  const int n = d.n, m = d.m, p = n + m, rec = g.rec = n * (1 + p);
  const int64_t G = g.G = d.seg_ptr[d.nseg];
  for (int64_t i = 0; i < G; ++i) if (d.src[i] < -1 || d.src[i] > d.N) TZ_FAIL_TO(err, TZ_ERR_INVALID, "src[%lld] out of range", (long long)i);
  g.lit.assign((size_t)std::max<int64_t>(G, 1) * rec, 0.0); g.srt.assign(g.lit.size(), 0.0);
  auto fill = [&](double* dst, int64_t gi) {
    for (int i = 0; i < n; ++i) { dst[i] = d.m0[(size_t)gi * n + i]; for (int c = 0; c < p; ++c) dst[n + i * p + c] = d.M[((size_t)gi * n + i) * p + c]; }
  };
  for (int64_t gi = 0; gi < G; ++gi) fill(&g.lit[(size_t)gi * rec], gi);
  // sorted by (tube, source) and cut into chunks
  g.seg_chunk_ptr.assign((size_t)d.nseg + 1, 0);
  int64_t pos = 0;
  for (int k = 0; k < d.nseg; ++k) {
    std::vector<int64_t> idx;
    for (int64_t gi = d.seg_ptr[k]; gi < d.seg_ptr[k + 1]; ++gi) idx.push_back(gi);
    std::stable_sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b2) { return d.src[a] < d.src[b2]; });
    size_t a = 0;
    while (a < idx.size()) {
      size_t b2 = a;
      while (b2 < idx.size() && d.src[idx[b2]] == d.src[idx[a]] && b2 - a < TZ_GS_CHUNK) ++b2;
      g.chunks.push_back(GsChunk{k, d.src[idx[a]], (int)pos, (int)(pos + (int64_t)(b2 - a))});
      for (size_t e = a; e < b2; ++e) fill(&g.srt[(size_t)pos++ * rec], idx[e]);
      a = b2;
    }
    g.seg_chunk_ptr[k + 1] = (int)g.chunks.size();
  }
  g.nchunk = (int)g.chunks.size();
  g.mfma = (p >= 3 && p <= 7);
  // one input (the reference's systems): a second copy of the stack holds only the n rows [m0 | M] -- 1 / (n + 1) fewer bytes and matrix
  // instructions -- and K g is formed in the kernel; it serves every batch except 33 .. 64 trajectories, where the extra vector
  // arithmetic of the narrow kernel costs more than the rows save (measured: LAB_NOTEBOOK.md, "K g formed in the kernel").
  g.rows_mf = (m == 1) ? n : p;
  if (g.mfma && !g.chunks.empty()) {
    g.mf = tz_genstack_plan_layout(d, g, p, &g.chunks_m);
    for (double v : g.mf) if (!std::isfinite(v)) TZ_FAIL_TO(err, TZ_ERR_INVALID, "non-finite generator entry");
    if (g.rows_mf != p) g.mfn = tz_genstack_plan_layout(d, g, g.rows_mf, nullptr);
  }
  if (g.chunks.empty()) g.chunks.push_back(GsChunk{0, -1, 0, 0});       // the kernels' table is never empty; nchunk stays 0
  if (d.cZ) {
    const size_t cnt = (size_t)d.nseg * d.N * n * p;
    for (size_t i = 0; i < cnt && !g.have_cZ; ++i) if (d.cZ[i] != 0.0) g.have_cZ = true;
  }
  return TZ_OK;
}
