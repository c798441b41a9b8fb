// Data contract between the host planner (tz_plan.h) and the kernels: the sizes, record formats and the LDS footprint both sides
// must agree on.  Plain C++, no HIP: the kernel headers include it, and so does the planner, which is compiled and tested on a CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define TZ_HD __host__ __device__
#else
#define TZ_HD
#endif

#define TZ_THREADS 256
#define TZ_NWAVES 4
#define TZ_NMAX 16         // max dim_x / dim_u of the MPC path (register arrays of the plant update, LDS slots of the closed-loop state);
#define TZ_MMAX 8          // K0 (tz_identify.hip.h) and the gain kernels (tz_gain.hip.h) keep their own limits of 8 / 4
#define TZ_PMAX 128        // highest supported power of M_K
#define TZ_ID_NMAX 8       // K0: dim_x <= 8, dim_u <= 4 (tile counts in tz_identify.hip.h)
#define TZ_ID_MMAX 4
#define TZ_GN_NMAX 8       // gain kernels: n <= 8

// Affine map rows over theta in ELL form: entry e of row r at [e * rows + r] (coalesced over rows), W entries per row, rows
// with fewer non-zeros padded with (0.0, column 0).  No row pointers: every load of a row is independent of the others.  An entry
// is one 16-byte record (value, byte offset of the theta entry, zero): one vector-memory instruction per non-zero.
struct __attribute__((aligned(16))) TzEllEnt { double val; unsigned off; unsigned pad; };

// H lives in LDS as tile rows of quads (4 column tiles); a quad is 4 matrix rows of 16 doubles padded to TZ_QROW = 17 so
// that neither the MFMA accumulator access (row-major inside the quad) nor the column access of the factorisation and the
// triangular solves runs into LDS bank conflicts (row stride 16 doubles = 32 banks collides 4- to 8-way).
#define TZ_QROW 17
#define TZ_QSTR (4 * TZ_QROW)
struct IpmItem { int I0, q0, nq, kptr, klen; };

#define TZ_KS_TZ 10        // most tile columns of the super-step Gram (tz_form_H_ksplit, tz_ipm.hip.h), i.e. nz <= 40

struct TzGUnit { int ib, jb, s0; };     // tile rows [ib, ib + U) x tile columns [jb, jb + U); s0: first super-step that touches tile column ib
// unit size of the blocked Gram by register budget (MINW = workgroups per CU the variant is compiled for: 2 -> 256 registers,
// 1 -> 512); the planner cuts its units with the same size
#define TZ_TT_GU(minw) ((minw) >= 2 ? 6 : 8)

// LDS footprint of tz_ipm_kernel in doubles.  hsize: doubles of the factor storage -- nquads * TZ_QSTR in the
// quad layout (nz <= 64), ntile * TS in the tile-triangle layout; the latter keeps 16 more doubles behind dinv for the factor of
// the diagonal tile being eliminated (tz_cholesky_tt).
TZ_HD inline size_t tz_ipm_lds_doubles(size_t hsize, int tt, int Tz, int nzp, int mip, int nklist, int ntheta, int ksplit, int ntube, int nell, int park = 0) {
  return (park ? 2 * (size_t)mip : 0) + (ksplit ? hsize : 0) + hsize + (size_t)Tz * 16 + (tt ? 16 : 0) + 14 * (size_t)nzp + (size_t)(mip + 4) + 32 + 2 + (size_t)((nklist + 1) / 2) + (size_t)ntheta + 4 * TZ_NMAX + (size_t)ntube + (size_t)nell;
}

#define TZ_GS_CHUNK 1024         // generators per workgroup (host plan)
#define TZ_GS_NARROW_SUB 2       // narrow kernel (few trajectories): blocks that share a chunk, each streaming its tiles once (measured at 32
                                 // trajectories, 636 chunks: 1 -> 0.0670 ms, 2 -> 0.0641 ms, 4 -> 0.120 ms: the un-overlapped prologue of short blocks)
struct GsChunk { int seg, src, g0, g1; };        // generators [g0, g1) of the SORTED stack: tube seg, source src (-1 none, 0 e0, 1 + j zeta_j)
struct GsChunkM { int seg, src, q0, nq; };       // groups [q0, q0 + nq) of 4 generators each (zero-padded), tube seg, source src
