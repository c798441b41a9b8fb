// CPU build of the host planner (tzddpc_amd/csrc/tz_plan.h): tests/test_host_plan.py compiles this with UBSan and the libstdc++
// assertions, builds plans for the descriptions the product sends and reads their scalars and tables back by name.
// Test infrastructure only.
#include "../../tzddpc_amd/csrc/tz_plan.h"
#include <cstring>

static TzPlan g_plan;
static TzGenstackPlan g_gs;
static std::string g_err;

#define SCALAR(obj, f) if (!strcmp(name, #f)) return (long long)(obj).f
#define TABLE(key, v) if (!strcmp(name, key)) { *count = (long long)(v).size(); *elem_bytes = (int)sizeof((v)[0]); return (v).data(); }

extern "C" {

const char* plan_error(void) { return g_err.c_str(); }
int plan_build(const tz_problem_desc* d) { g_err.clear(); return tz_plan_build(*d, g_plan, g_err); }
int genstack_build(const tz_genstack_desc* d) { g_err.clear(); return tz_genstack_plan_build(*d, g_gs, g_err); }

long long layout_const(const char* name) {
#define CONST(c) if (!strcmp(name, #c)) return c
  CONST(TZ_THREADS); CONST(TZ_NWAVES); CONST(TZ_QSTR); CONST(TZ_KS_TZ); CONST(TZ_GS_CHUNK); CONST(TZ_GS_NARROW_SUB);
  if (!strcmp(name, "TZ_TT_GU1")) return TZ_TT_GU(1);
  if (!strcmp(name, "TZ_TT_GU2")) return TZ_TT_GU(2);
  return -1;
}

long long lds_doubles(long long hsize, int tt, int Tz, int nzp, int mip, int nklist, int ntheta, int ksplit, int ntube, int nell, int park) {
  return (long long)tz_ipm_lds_doubles((size_t)hsize, tt, Tz, nzp, mip, nklist, ntheta, ksplit, ntube, nell, park);
}

long long plan_scalar(const char* name) {
  SCALAR(g_plan, nzp); SCALAR(g_plan, mip); SCALAR(g_plan, Tz); SCALAR(g_plan, Kc); SCALAR(g_plan, nquads); SCALAR(g_plan, nklist);
  SCALAR(g_plan, nP); SCALAR(g_plan, maxr); SCALAR(g_plan, ncg); SCALAR(g_plan, tt); SCALAR(g_plan, staircase); SCALAR(g_plan, ksplit);
  SCALAR(g_plan, TS); SCALAR(g_plan, ntile); SCALAR(g_plan, gu); SCALAR(g_plan, hsize); SCALAR(g_plan, nell); SCALAR(g_plan, ntube);
  SCALAR(g_plan, lds_bytes); SCALAR(g_plan, wgs_per_cu); SCALAR(g_plan, lean_epilogue); SCALAR(g_plan, fused);
  SCALAR(g_plan, mfma_gram); SCALAR(g_plan, mfma_chol); SCALAR(g_plan, mfma_issued);
  SCALAR(g_plan, eg.L); SCALAR(g_plan, eg.VL); SCALAR(g_plan, et.L); SCALAR(g_plan, et.VL);
  SCALAR(g_plan, q.rows); SCALAR(g_plan, q.W); SCALAR(g_plan, h.rows); SCALAR(g_plan, h.W); SCALAR(g_plan, par.rows); SCALAR(g_plan, par.W);
  return -1;
}

const void* plan_table(const char* name, long long* count, int* elem_bytes) {
  TABLE("permc", g_plan.permc) TABLE("permr", g_plan.permr) TABLE("vpos", g_plan.vpos) TABLE("P", g_plan.P) TABLE("Gp", g_plan.Gp)
  TABLE("klist", g_plan.klist) TABLE("item_ptr", g_plan.item_ptr) TABLE("smask", g_plan.smask) TABLE("items", g_plan.items)
  TABLE("eg.ent", g_plan.eg.ent) TABLE("eg.seg", g_plan.eg.seg) TABLE("eg.val", g_plan.eg.val) TABLE("eg.idx", g_plan.eg.idx)
  TABLE("et.ent", g_plan.et.ent) TABLE("et.seg", g_plan.et.seg) TABLE("et.val", g_plan.et.val) TABLE("et.idx", g_plan.et.idx)
  TABLE("q.ent", g_plan.q.ent) TABLE("q.c0", g_plan.q.c0) TABLE("h.ent", g_plan.h.ent) TABLE("h.c0", g_plan.h.c0)
  TABLE("par.ent", g_plan.par.ent) TABLE("par.c0", g_plan.par.c0)
  TABLE("CKpow", g_plan.CKpow) TABLE("Ttube", g_plan.Ttube) TABLE("act_scale", g_plan.act_scale) TABLE("row_of", g_plan.row_of)
  TABLE("rec0", g_plan.rec0) TABLE("recx", g_plan.recx) TABLE("recy", g_plan.recy)
  TABLE("shift_var", g_plan.shift_var) TABLE("shift_row", g_plan.shift_row) TABLE("shift_xs", g_plan.shift_xs) TABLE("shift_ls", g_plan.shift_ls)
  TABLE("gunits", g_plan.gunits) TABLE("gunit_ptr", g_plan.gunit_ptr)
  *count = -1; *elem_bytes = 0;
  return nullptr;
}

long long genstack_scalar(const char* name) {
  SCALAR(g_gs, rec); SCALAR(g_gs, nchunk); SCALAR(g_gs, G); SCALAR(g_gs, mfma); SCALAR(g_gs, rows_mf); SCALAR(g_gs, have_cZ);
  return -1;
}

const void* genstack_table(const char* name, long long* count, int* elem_bytes) {
  TABLE("lit", g_gs.lit) TABLE("srt", g_gs.srt) TABLE("chunks", g_gs.chunks) TABLE("seg_chunk_ptr", g_gs.seg_chunk_ptr)
  TABLE("mf", g_gs.mf) TABLE("mfn", g_gs.mfn) TABLE("chunks_m", g_gs.chunks_m)
  *count = -1; *elem_bytes = 0;
  return nullptr;
}

}  // extern "C"
