// dvm_slam_amd/csrc/pg_kernels.hip -- Optimizer::OptimizeEssentialGraph on the device, FP64, for gfx950 (driver: pg_solver.cpp):
//   k_pg_edge       per-edge error log(C * Si * Sj^-1), chi2 partial, numeric 7x7 Jacobians
//   k_reduce_sum    the partials of a pass in a fixed order
//   k_zero_tiles, k_pg_blocks, k_pg_rhs, k_pad_identity   the 7-DoF system in the tile solver's layout (tile_system.h; solved by tile_launch_cholesky_solve)
//   k_pg_update     oplus and the computeScale partial
// g2o::Sim3 is sim3_f64.h's.  Launchers: ba_kernels.h.
#include <hip/hip_runtime.h>

#include "ba_kernels.h"
#include "sim3_f64.h"

namespace dvm {

// ---------------------------------------------------------------------------------- essential graph
// Optimizer::OptimizeEssentialGraph numerics (reference src/Optimizer.cc:1389-1652): VertexSim3Expmap + EdgeSim3
// (types_seven_dof_expmap.h:93-117), numeric Jacobians as g2o takes them (base_binary_edge.hpp:131-205).
__device__ void pg_edge_error(const Sim3d& C, const Sim3d& Si, const Sim3d& Sj, double* e) {   // log(C * v1 * v2^-1)
  Sim3d Sji, t1, t2;
  sim3_inv(Sj, Sji);
  sim3_mul(C, Si, t1);
  sim3_mul(t1, Sji, t2);
  sim3_log(t2, e);
}
// thread per edge: error, chi2 partial; JAC: the two 7x7 numeric Jacobians (14 columns x 2 perturbed error evaluations)
template <bool JAC>
__global__ void __launch_bounds__(256) k_pg_edge(PgView G) {
  __shared__ double red[256];
  const int k = blockIdx.x * 256 + threadIdx.x;
  double chi = 0;
  if (k < G.E) {
    const int vi = G.ev[2 * k], vj = G.ev[2 * k + 1];
    Sim3d C, Si, Sj;
    sim3_load(G.emeas + 8 * (size_t)k, C); sim3_load(G.S + 8 * (size_t)vi, Si); sim3_load(G.S + 8 * (size_t)vj, Sj);
    double e[7];
    pg_edge_error(C, Si, Sj, e);
    // e_err belongs to the linearisation: b = -J^T e is rebuilt from it in EVERY trial of the iteration (k_pg_rhs), so the chi2-only
    // pass at a trial state must leave it alone -- g2o builds b once per iteration (a rejected trial used to leave its errors here)
    for (int a = 0; a < 7; a++) { if (JAC) G.e_err[7 * (size_t)k + a] = e[a]; chi += e[a] * e[a]; }
    if (JAC) {
      for (int side = 0; side < 2; side++) {
        const int v = side ? vj : vi;
        double* J = G.e_J + (size_t)k * 98 + 49 * side;
        if (G.vidx[v] < 0) { for (int a = 0; a < 49; a++) J[a] = 0; continue; }
        const Sim3d& X = side ? Sj : Si;
        for (int d = 0; d < 7; d++) {
          double e1[7], e2[7];
          for (int sgn = 0; sgn < 2; sgn++) {
            double u[7] = {0, 0, 0, 0, 0, 0, 0};
            u[d] = sgn ? -1e-9 : 1e-9;
            if (G.fix_scale) u[6] = 0;
            Sim3d Ex, Xp;
            sim3_exp(u, Ex);
            sim3_mul(Ex, X, Xp);
            pg_edge_error(C, side ? Si : Xp, side ? Xp : Sj, sgn ? e2 : e1);
          }
          for (int a = 0; a < 7; a++) J[7 * a + d] = (1.0 / (2 * 1e-9)) * (e1[a] - e2[a]);
        }
      }
    }
  }
  red[threadIdx.x] = chi;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) G.partial[blockIdx.x] = red[0];
}
// Sum `n` partials in a fixed order into out[slot]; single workgroup.
__global__ void __launch_bounds__(256) k_reduce_sum(const double* __restrict__ partial, int n, double* __restrict__ out, int slot) {
  __shared__ double s[256];
  double acc = 0;
  for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
  s[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[slot] = s[0];
}

// 64 threads per non-zero 7x7 block (a >= b): H_ab = sum over its contributions J_a^T J_b (+ lambda on the diagonal),
// fixed order, written into the tile-space matrix
__global__ void __launch_bounds__(256) k_pg_blocks(PgView G, TileSystem T) {
  const int blk = blockIdx.x * 4 + (threadIdx.x >> 6), t = threadIdx.x & 63;
  if (blk >= G.nblk || t >= 49) return;
  const int r = t / 7, c = t % 7;
  const int a = G.blk_a[blk], b = G.blk_b[blk];
  double acc = 0;
  for (int i = G.blk_start[blk]; i < G.blk_start[blk + 1]; i++) {
    const int w = G.blk_contrib[i];
    const double* Ja = G.e_J + (size_t)(w >> 2) * 98 + 49 * ((w >> 1) & 1);
    const double* Jb = G.e_J + (size_t)(w >> 2) * 98 + 49 * (w & 1);
    double h = 0;
#pragma unroll
    for (int k = 0; k < 7; k++) h += Ja[7 * k + r] * Jb[7 * k + c];
    acc += h;
  }
  if (a == b && r == c) acc += *G.lambda;
  const int ra = (a / T.per_tile) * 64 + (a % T.per_tile) * T.dof, rb = (b / T.per_tile) * 64 + (b % T.per_tile) * T.dof;
  T.S[(size_t)(ra + r) * T.ldS + rb + c] = acc;
}
// clears the structurally non-zero tiles of S (a trial rebuilds them); everything else is never touched and stays zero
// from the allocation-time memset: 197 of 1 326 tiles = 6 MB instead of 85 MB at 500 keyframes
__global__ void __launch_bounds__(256) k_zero_tiles(double* __restrict__ S, int ldS, const int32_t* __restrict__ nz) {
  const int ti = nz[2 * blockIdx.x], tj = nz[2 * blockIdx.x + 1];
  double* base = S + (size_t)ti * 64 * ldS + tj * 64;
  for (int i = threadIdx.x; i < 64 * 32; i += 256) {
    const int r = i >> 5, c2 = i & 31;
    reinterpret_cast<double2*>(base + (size_t)r * ldS)[c2] = make_double2(0.0, 0.0);
  }
}

// identity on the padding rows of the tiled system (rows 60..63 of every tile, cameras beyond nfree in the last tile)
__global__ void __launch_bounds__(256) k_pad_identity(TileSystem V) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= V.n_pad) return;
  const int w = r & 63;
  if (w >= V.per_tile * V.dof || (r >> 6) * V.per_tile + w / V.dof >= V.nfree) V.S[(size_t)r * V.ldS + r] = 1.0;
}

// thread per free vertex: b_v = - sum J_v^T e  -> compact copy (computeScale) and the augmented rhs row
__global__ void __launch_bounds__(256) k_pg_rhs(PgView G, TileSystem T) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= G.nfree) return;
  double b[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = G.v_start[p]; i < G.v_start[p + 1]; i++) {
    const int w = G.v_contrib[i];
    const double* J = G.e_J + (size_t)(w >> 1) * 98 + 49 * (w & 1);
    const double* e = G.e_err + 7 * (size_t)(w >> 1);
    for (int r = 0; r < 7; r++) {
      double g = 0;
#pragma unroll
      for (int a = 0; a < 7; a++) g += J[7 * a + r] * (-e[a]);
      b[r] += g;
    }
  }
  const int row = (p / T.per_tile) * 64 + (p % T.per_tile) * T.dof;
  for (int r = 0; r < 7; r++) { G.bp[7 * (size_t)p + r] = b[r]; T.S[(size_t)T.n_pad * T.ldS + row + r] = b[r]; }
  if (p == 0) T.S[(size_t)T.n_pad * T.ldS + T.n_pad] = 1e200;
}
// thread per free vertex: oplus (S <- Sim3(x) * S) and the computeScale partial sum x^T (lambda x + b)
__global__ void __launch_bounds__(256) k_pg_update(PgView G, TileSystem T) {
  __shared__ double red[256];
  const int p = blockIdx.x * 256 + threadIdx.x;
  double sc = 0;
  if (p < G.nfree) {
    const double lambda = *G.lambda;
    double u[7];
    for (int r = 0; r < 7; r++) { u[r] = T.x[7 * (size_t)p + r]; sc += u[r] * (lambda * u[r] + G.bp[7 * (size_t)p + r]); }
    if (G.fix_scale) u[6] = 0;
    double* Sp = G.S + 8 * (size_t)G.free_v[p];
    Sim3d X, Ex, Xn;
    sim3_load(Sp, X);
    sim3_exp(u, Ex);
    sim3_mul(Ex, X, Xn);
    Sp[0] = Xn.q[0]; Sp[1] = Xn.q[1]; Sp[2] = Xn.q[2]; Sp[3] = Xn.q[3]; Sp[4] = Xn.t[0]; Sp[5] = Xn.t[1]; Sp[6] = Xn.t[2]; Sp[7] = Xn.s;
  }
  red[threadIdx.x] = sc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) G.partial[blockIdx.x] = red[0];
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

void pg_launch_edge_eval(hipStream_t s, const PgView& G, bool jac, double* d_scalars, int slot) {
  const int nb = cdiv(G.E, 256);
  if (jac) hipLaunchKernelGGL(k_pg_edge<true>, dim3(nb), dim3(256), 0, s, G);
  else hipLaunchKernelGGL(k_pg_edge<false>, dim3(nb), dim3(256), 0, s, G);
  hipLaunchKernelGGL(k_reduce_sum, dim3(1), dim3(256), 0, s, G.partial, nb, d_scalars, slot);
}
void pg_launch_build(hipStream_t s, const PgView& G, const TileSystem& T) {
  hipLaunchKernelGGL(k_zero_tiles, dim3(T.n_nz), dim3(256), 0, s, T.S, T.ldS, T.nz_tiles);
  hipLaunchKernelGGL(k_pg_blocks, dim3(cdiv(G.nblk, 4)), dim3(256), 0, s, G, T);
  hipLaunchKernelGGL(k_pg_rhs, dim3(cdiv(G.nfree, 256)), dim3(256), 0, s, G, T);
  hipLaunchKernelGGL(k_pad_identity, dim3(cdiv(T.n_pad, 256)), dim3(256), 0, s, T);
}
void pg_launch_update(hipStream_t s, const PgView& G, const TileSystem& T, double* d_scalars, int slot_scale) {
  const int nb = cdiv(G.nfree, 256);
  hipLaunchKernelGGL(k_pg_update, dim3(nb), dim3(256), 0, s, G, T);
  hipLaunchKernelGGL(k_reduce_sum, dim3(1), dim3(256), 0, s, G.partial, nb, d_scalars, slot_scale);
}

}  // namespace dvm
