// bh_energy.hip — system energy diagnostics: one deterministic fp64 reduction over the bodies and their potentials
// (force_pot_kernel, bh_force.hip), and the potentials in caller order.
//
// Every workgroup sums a fixed, strided share of the bodies in a fixed order (grid and shares depend on n only), writes
// its BH_ENERGY_SUMS partials, and the last workgroup to finish (bh_last_block, bh_internal.h: fence-free hand-off) adds
// the partials in workgroup order.  No floating-point atomics: two calls on the same state return the same bits.
#include "bh_internal.h"

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ void block_sum(double (*red)[kThreads], double* v) {
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < BH_ENERGY_SUMS; q++) red[q][t] = v[q];
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int q = 0; q < BH_ENERGY_SUMS; q++) red[q][t] += red[q][t + s];
    }
    __syncthreads();
  }
}

// sums over body i: m, m |v|^2, m phi, m v, m (x cross v), m x — in fp64 from the fp32 state
__global__ __launch_bounds__(kThreads) void energy_sums_kernel(const float4* __restrict__ posm,
                                                               const float4* __restrict__ velid,
                                                               const float* __restrict__ pot, int n,
                                                               double* __restrict__ part, u32* __restrict__ cnt) {
  __shared__ double red[BH_ENERGY_SUMS][kThreads];
  __shared__ int last;
  double v[BH_ENERGY_SUMS];
#pragma unroll
  for (int q = 0; q < BH_ENERGY_SUMS; q++) v[q] = 0.0;
  const int stride = gridDim.x * kThreads;
  for (int i = blockIdx.x * kThreads + (int)threadIdx.x; i < n; i += stride) {
    const float4 p = posm[i], u = velid[i];
    const double m = p.w, x = p.x, y = p.y, z = p.z, vx = u.x, vy = u.y, vz = u.z;
    v[0] += m;
    v[1] += m * (vx * vx + vy * vy + vz * vz);
    v[2] += m * (double)pot[i];
    v[3] += m * vx;
    v[4] += m * vy;
    v[5] += m * vz;
    v[6] += m * (y * vz - z * vy);
    v[7] += m * (z * vx - x * vz);
    v[8] += m * (x * vy - y * vx);
    v[9] += m * x;
    v[10] += m * y;
    v[11] += m * z;
  }
  block_sum(red, v);
  const int t = threadIdx.x;
  if (t < BH_ENERGY_SUMS) {
    __hip_atomic_store(reinterpret_cast<u64*>(part) + (size_t)blockIdx.x * BH_ENERGY_SUMS + t,
                       (u64)__double_as_longlong(red[t][0]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bh_published();
  }
  if (t == 0) last = bh_last_block(cnt, blockIdx.x, gridDim.x) ? 1 : 0;
  __syncthreads();
  if (!last) return;
  // the last workgroup: the partials in workgroup order (thread t: workgroups t, t + 256, ..., then the tree above)
#pragma unroll
  for (int q = 0; q < BH_ENERGY_SUMS; q++) v[q] = 0.0;
  for (int b = t; b < (int)gridDim.x; b += kThreads) {
    const u64* row = reinterpret_cast<const u64*>(part) + (size_t)b * BH_ENERGY_SUMS;
#pragma unroll
    for (int q = 0; q < BH_ENERGY_SUMS; q++)
      v[q] += __longlong_as_double((long long)__hip_atomic_load(row + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
  __syncthreads();  // red[] is reused
  block_sum(red, v);
  if (t < BH_ENERGY_SUMS) part[(size_t)BH_ENERGY_BLOCKS * BH_ENERGY_SUMS + t] = red[t][0];
}

__global__ __launch_bounds__(256) void unpack_f32_kernel(const float* __restrict__ a, const float4* __restrict__ velid,
                                                         int n, float* __restrict__ s) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  s[__float_as_int(velid[i].w)] = a[i];
}

// bh_rank_step_energy: this rank's row of the energy all-gather (BH_ENERGY_ROW doubles) — its sums (zero when sums is
// null: the energy part failed before them), its sticky flags, its local-failure status, its body count
__global__ void energy_row_kernel(const double* __restrict__ sums, const bh_devinfo* __restrict__ info, int fail,
                                  int n, double* __restrict__ row) {
  const int t = threadIdx.x;
  if (t >= BH_ENERGY_ROW) return;
  double v = 0.0;
  if (t < BH_ENERGY_SUMS)
    v = sums ? sums[t] : 0.0;
  else if (t == BH_ENERGY_SUMS)
    v = (double)info->flags;
  else if (t == BH_ENERGY_SUMS + 1)
    v = (double)fail;
  else if (t == BH_ENERGY_SUMS + 2)
    v = (double)n;
  row[t] = v;
}

}  // namespace

hipError_t bhk_energy_sums(bh_ctx* c) {
  const int n = c->n;
  const int per = (n + kThreads - 1) / kThreads;
  const int blocks = per < 1 ? 1 : (per < BH_ENERGY_BLOCKS ? per : BH_ENERGY_BLOCKS);  // (a rank may hold no body)
  energy_sums_kernel<<<blocks, kThreads, 0, c->stream>>>(c->posm[c->cur], c->velid[c->cur], c->pot, n, c->en_part,
                                                        c->en_cnt);
  return hipGetLastError();
}

hipError_t bhk_unpack_pot(bh_ctx* c) {
  const int n = c->n;
  unpack_f32_kernel<<<(n + 255) / 256, 256, 0, c->stream>>>(c->pot, c->velid[c->cur], n, c->stage_buf);
  return hipGetLastError();
}

hipError_t bhk_energy_row(bh_ctx* c, int fail, void* row) {
  const double* sums = c->en_part ? c->en_part + (size_t)BH_ENERGY_BLOCKS * BH_ENERGY_SUMS : nullptr;
  energy_row_kernel<<<1, 64, 0, c->stream>>>(fail ? nullptr : sums, c->info, fail, c->n, (double*)row);
  return hipGetLastError();
}
