// Device code of the step tail (the split-K reductions of both Del weights with Adam, the folded layer-1 column job, the loss
// finalize), shared by the tail kernels of rows_gemm.hip and by the hosted aggregation launch of spmm.hip: the arithmetic exists once.
#pragma once
#include "common.h"

namespace gd {

// The launch-sized tail of a training step in ONE launch: the split-K reductions of both Del weights (block order, the
// association of wgrad_reduce_adam_kernel - bit-identical results) each with its Adam update, and the loss finalize (per-block
// loss partials -> history ring, ring position, iteration counter).  Three launches and two kernel boundaries less per step.
// The Adam blocks need the step number t = *iter + 1 and the finalize block advances *iter in the same launch: every Adam block
// reads the counter FIRST (a returning device-scope atomic) and then checks in on `arrive`; the finalize thread writes the counter
// only after all of them have checked in, and resets `arrive` for the next launch.  The grid (n_elem / 64 blocks per weight + 1:
// 321 at 128 x 128 + 64 x 64) is a fraction of the resident set, so every block is scheduled while the one thread waits.
struct TailJob {
  const float* partials; int32_t n_part, n_elem, accumulate;
  float* dw; float* param; float* m; float* v;
};
struct TailFin {
  const float* p1; int32_t n1; const float* p2; int32_t n2;
  float* hist; int32_t capacity; int32_t* pos; int32_t* iter; int32_t* arrive;
};
struct TailFold1 { const float* colsum; const float* w1; const float* b1; float* wf; float* bf; };

__device__ __forceinline__ int32_t tail_check_in(const TailFin& fin) {
  int32_t t = atomicAdd(fin.iter, 0);                 // the counter as the L2 holds it, before this block checks in
  asm volatile("" : "+v"(t));
  atomicAdd(fin.arrive + (t < 0 ? 1 : 0), 1);         // (address depends on t: the check-in cannot pass the read)
  return t + 1;
}

// One block of a split-K reduction + Adam job (blk: its index inside the job): reduces its 64 elements over the partial matrices in
// block order and steps Adam on them with the step number in *t_sh (thread 0 wrote it before the call; read behind the barrier).
__device__ __forceinline__ void tail_reduce_adam(const TailJob& j, int blk, float4 (*red)[16], const int32_t* t_sh, double lr, double beta1,
                                                 double beta2, double eps) {
  const int tid = threadIdx.x;
  const int vv = tid & 15, slice = tid >> 4;
  const int e4 = blk * 16 + vv;
  const int n4 = j.n_elem >> 2;
  float4 s0 = f4_zero(), s1 = f4_zero(), s2 = f4_zero(), s3 = f4_zero();
  if (e4 < n4) {
    int b = slice;
    for (; b + 48 < j.n_part; b += 64) {
      const float4 p0 = reinterpret_cast<const float4*>(j.partials + (int64_t)b * j.n_elem)[e4];
      const float4 p1 = reinterpret_cast<const float4*>(j.partials + (int64_t)(b + 16) * j.n_elem)[e4];
      const float4 p2 = reinterpret_cast<const float4*>(j.partials + (int64_t)(b + 32) * j.n_elem)[e4];
      const float4 p3 = reinterpret_cast<const float4*>(j.partials + (int64_t)(b + 48) * j.n_elem)[e4];
      s0 = f4_add(s0, p0); s1 = f4_add(s1, p1); s2 = f4_add(s2, p2); s3 = f4_add(s3, p3);
    }
    for (; b < j.n_part; b += 16) s0 = f4_add(s0, reinterpret_cast<const float4*>(j.partials + (int64_t)b * j.n_elem)[e4]);
  }
  red[slice][vv] = f4_add(f4_add(s0, s1), f4_add(s2, s3));
  __syncthreads();
  if (slice == 0 && e4 < n4) {
    float4 t4 = j.accumulate ? reinterpret_cast<float4*>(j.dw)[e4] : f4_zero();
#pragma unroll
    for (int i = 0; i < 16; ++i) t4 = f4_add(t4, red[i][vv]);
    reinterpret_cast<float4*>(j.dw)[e4] = t4;
    const AdamScalars sc = adam_scalars(lr, beta1, beta2, eps, *t_sh);
    float4 p4 = reinterpret_cast<float4*>(j.param)[e4], m4 = reinterpret_cast<float4*>(j.m)[e4],
           v4 = reinterpret_cast<float4*>(j.v)[e4];
    adam_update(p4.x, m4.x, v4.x, t4.x, sc);
    adam_update(p4.y, m4.y, v4.y, t4.y, sc);
    adam_update(p4.z, m4.z, v4.z, t4.z, sc);
    adam_update(p4.w, m4.w, v4.w, t4.w, sc);
    reinterpret_cast<float4*>(j.param)[e4] = p4;
    reinterpret_cast<float4*>(j.m)[e4] = m4;
    reinterpret_cast<float4*>(j.v)[e4] = v4;
  }
}

// The same block inside a tail launch: reads the counter, checks in, then the job.
__device__ __forceinline__ void tail_job_block(const TailJob& j, int blk, const TailFin& fin, float4 (*red)[16], int32_t* t_sh, double lr,
                                               double beta1, double beta2, double eps) {
  if (threadIdx.x == 0) *t_sh = tail_check_in(fin);
  tail_reduce_adam(j, blk, red, t_sh, lr, beta1, beta2, eps);
}

// The sums of the finalize (same arithmetic and order as loss_finalize_kernel) and the history row.  Ends with a barrier.
__device__ __forceinline__ void tail_finalize_sums(const TailFin& fin, float (*fred)[256]) {
  const int tid = threadIdx.x;
  float a = 0.f, b = 0.f, c = 0.f, d = 0.f;
  for (int i = tid; i < fin.n1; i += 256) { a += fin.p1[2 * i]; b += fin.p1[2 * i + 1]; }
  for (int i = tid; i < fin.n2; i += 256) { c += fin.p2[2 * i]; d += fin.p2[2 * i + 1]; }
  fred[0][tid] = a; fred[1][tid] = b; fred[2][tid] = c; fred[3][tid] = d;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int q = 0; q < 4; ++q) fred[q][tid] += fred[q][tid + off];
    }
    __syncthreads();
  }
  if (tid < 4) fin.hist[(int64_t)(*fin.pos) * 4 + tid] = fred[tid][0];
  __syncthreads();
}

// The finalize block of a tail launch; n_wait: the blocks that check in.
__device__ __forceinline__ void tail_finalize_block(const TailFin& fin, float (*fred)[256], int n_wait) {
  tail_finalize_sums(fin, fred);
  if (threadIdx.x == 0) {
    while (atomicAdd(fin.arrive, 0) < n_wait) __builtin_amdgcn_s_sleep(8);
    *fin.arrive = 0;
    *fin.pos = (*fin.pos + 1) % fin.capacity;
    atomicAdd(fin.iter, 1);
  }
}

// One 64-long fmaf chain of a 128 x 128 product, in order: sum over k = k0 .. k0 + 63 of mat[k * SK] * vec[k] (mat already offset
// to the thread's row or column).  SK = 129: the LDS image of W1, 128: W1 or its transposed copy in global memory.
template <int SK>
__device__ __forceinline__ float tail_chain64(const float* mat, const float* vec, int k0) {
  float acc = 0.f;
#pragma unroll 16
  for (int k = k0; k < k0 + 64; ++k) acc = fmaf(mat[k * SK], vec[k], acc);
  return acc;
}

// Column c of the layer-1 fold from column c of W_D (wd_col[128] in LDS): Wf[:, c] = W1^T W_D[:, c] and bf[c] = b1 . W_D[:, c], with
// W1 ([128 out, 128 in], conv1's Linear) as w1m[j * LD + i]: LD = 129 its LDS image, LD = 128 the weight itself in global memory.
// 256 threads: thread (i = tid & 127, half = tid >> 7) takes j = 64 half .. 64 half + 63 in order (one fmaf chain), the halves are
// added low + high; bf: a fixed tree over the 128 products.  scr: 256 floats of LDS.  Ends with a barrier.
template <int LD>
__device__ __forceinline__ void fold1_column(const float* w1m, const float* __restrict__ b1, const float* wd_col, int c, float* scr,
                                             float* __restrict__ wf, float* __restrict__ bf) {
  const int tid = threadIdx.x, i = tid & 127, hf = tid >> 7;
  scr[tid] = tail_chain64<LD>(w1m + i, wd_col, 64 * hf);
  __syncthreads();
  if (tid < 128) wf[(int64_t)tid * 128 + c] = scr[tid] + scr[tid + 128];
  __syncthreads();
  scr[tid] = tid < 128 ? b1[tid] * wd_col[tid] : 0.f;
  __syncthreads();
  for (int off = 64; off > 0; off >>= 1) {
    if (tid < off) scr[tid] += scr[tid + off];
    __syncthreads();
  }
  if (tid == 0) bf[c] = scr[0];
  __syncthreads();
}

// W1 into its LDS image in two halves, so that a caller can keep the 16 loads in flight under other work: 256 threads x 16 float4.
__device__ __forceinline__ void fold1_fetch_w1(const float* __restrict__ w1, float4 (&r)[16]) {
#pragma unroll
  for (int it = 0; it < 16; ++it) r[it] = reinterpret_cast<const float4*>(w1)[threadIdx.x + 256 * it];
}
__device__ __forceinline__ void fold1_store_w1(const float4 (&r)[16], float* w1s) {
#pragma unroll
  for (int it = 0; it < 16; ++it) {
    const int e = threadIdx.x + 256 * it;
    float* dst = w1s + (e >> 5) * 129 + (e & 31) * 4;
    dst[0] = r[it].x; dst[1] = r[it].y; dst[2] = r[it].z; dst[3] = r[it].w;
  }
}

// Job 1 of the tail of the step whose layer 1 is folded into W_D1 (d1 = 128): one block per COLUMN c of W_D1, every quantity being
// column-local:
//     G[:, c] = sum over the partial matrices (transposed: [slot][c][i]) in a fixed association (eight chains per slice of the
//               slots, added pairwise, then the 8 slices in order);   s[c] = sum of the column-sum partials (fixed tree)
//     dW[:, c] = W1 G[:, c] + b1 s[c] -> dw;   Adam on W_D1[:, c];   Wf[:, c], bf[c] of the NEXT step from the updated column.
// The step number is in *t_sh (thread 0 wrote it before the call).  IMAGE: W1 goes into the LDS image w1s ([128][129], 66 KB of
// dynamic LDS) under the reduction and both products read it there, eight partial rows in flight per thread.  Not IMAGE (a block
// inside a launch whose LDS size belongs to other blocks): the products read W1 from global memory, where it is L2-resident -
// dW's thread j the transposed copy w1t[i][j], the fold column's thread i W1[j][i] itself, both coalesced - and four partial rows
// are in flight; the accumulators, and so every association, are the same.
// LDS: red8 [8][32] float4, fred [4][256], gcol / wd_col [128].
template <bool IMAGE>
__device__ __forceinline__ void tail_fold1_column_block(const TailJob& j1, const TailFold1& fo, const float* __restrict__ w1t, int c,
                                                        float* w1s, float4* red8, float (*fred)[256], float* gcol, float* wd_col,
                                                        const int32_t* t_sh, double lr, double beta1, double beta2, double eps) {
  constexpr int D = 128;
  constexpr int F = IMAGE ? 8 : 4;                                   // partial rows in flight per thread
  const int tid = threadIdx.x;
  float4 w1r[IMAGE ? 16 : 1];
  if constexpr (IMAGE) fold1_fetch_w1(fo.w1, w1r);                   // (in flight under the reduction; stored behind it)
  // ---- G[:, c]: 8 slices of the slots x 32 float4
  {
    const int vv = tid & 31, slice = tid >> 5;
    const float4* src = reinterpret_cast<const float4*>(j1.partials + (int64_t)c * D) + vv;
    const int64_t pitch4 = (int64_t)D * D / 4;
    float4 sa[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) sa[q] = f4_zero();
    int b = slice;
    for (; b + 56 < j1.n_part; b += 64) {
#pragma unroll
      for (int q0 = 0; q0 < 8; q0 += F) {
        float4 pv[F];
#pragma unroll
        for (int q = 0; q < F; ++q) pv[q] = src[(b + 8 * (q0 + q)) * pitch4];
#pragma unroll
        for (int q = 0; q < F; ++q) sa[q0 + q] = f4_add(sa[q0 + q], pv[q]);
        if constexpr (!IMAGE) __builtin_amdgcn_sched_barrier(0);    // (or the scheduler puts all eight loads in flight again)
      }
    }
    for (; b < j1.n_part; b += 8) sa[0] = f4_add(sa[0], src[b * pitch4]);
    red8[slice * 32 + vv] = f4_add(f4_add(f4_add(sa[0], sa[1]), f4_add(sa[2], sa[3])), f4_add(f4_add(sa[4], sa[5]), f4_add(sa[6], sa[7])));
    float cs = 0.f;
    for (int q = tid; q < j1.n_part; q += 256) cs += fo.colsum[(int64_t)q * D + c];
    fred[0][tid] = cs;
    if constexpr (IMAGE) fold1_store_w1(w1r, w1s);
    __syncthreads();
    if (tid < 32) {
      float4 t4 = red8[tid];
#pragma unroll
      for (int i = 1; i < 8; ++i) t4 = f4_add(t4, red8[i * 32 + tid]);
      reinterpret_cast<float4*>(gcol)[tid] = t4;
    }
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) fred[0][tid] += fred[0][tid + off];
      __syncthreads();
    }
  }
  // ---- dW[:, c] = W1 G[:, c] + b1 s[c]; Adam on the column
  {
    const int j = tid & 127, hf = tid >> 7;
    fred[1][tid] = IMAGE ? tail_chain64<1>(w1s + j * 129, gcol, 64 * hf) : tail_chain64<D>(w1t + j, gcol, 64 * hf);
    __syncthreads();
    if (tid < D) {
      const float g = fmaf(fo.b1[tid], fred[0][0], fred[1][tid] + fred[1][tid + 128]);
      const int64_t e = (int64_t)tid * D + c;
      j1.dw[e] = g;
      const AdamScalars sc = adam_scalars(lr, beta1, beta2, eps, *t_sh);
      float pv = j1.param[e], mv = j1.m[e], vv = j1.v[e];
      adam_update(pv, mv, vv, g, sc);
      j1.param[e] = pv; j1.m[e] = mv; j1.v[e] = vv;
      wd_col[tid] = pv;
    }
    __syncthreads();
  }
  if constexpr (IMAGE) fold1_column<129>(w1s, fo.b1, wd_col, c, fred[2], fo.wf, fo.bf);
  else fold1_column<D>(fo.w1, fo.b1, wd_col, c, fred[2], fo.wf, fo.bf);
}

// ---------------------------------------------------------------------------------------------
// The tail's jobs as the first blocks of another kernel's grid (the hosted wide aggregation of spmm.hip): `nh` blocks (a multiple of
// 8) in front of the host's own, [0, n1b) the W_D1 column blocks (n1b = 128, or 0 without job 1), [n1b, n1b + nb2) the W_D2 blocks
// (nb2 = 0 without job 2), the rest idle.  No block waits for another.  Every job block reads the iteration counter first (a
// returning atomic).  In a launch WITH job 2 - the one whose finalize advances the counter - every job block, of either job, adds 1
// to `arrive` when its work is done, and the block whose add returns n1b + nb2 - 1 - the last one, whichever it is - runs the
// finalize: it tells its threads through LDS, forms the loss sums, writes the history row, resets `arrive` and advances the ring
// position and the counter.  By then every job block of the launch has read the counter: the read has returned before the same
// thread's add is issued.  In a launch with job 1 alone nothing advances the counter and nobody checks in.  Nothing depends on the
// order in which blocks are dispatched.
struct TailHost {
  TailJob j1, j2; TailFin fin; TailFold1 fo; const float* w1t;
  int32_t n1b, nb2, nh;
  double lr, beta1, beta2, eps;
};

__device__ __forceinline__ void tail_host_block(const TailHost& h, int blk) {
  __shared__ float4 red[16][16];
  __shared__ float fred[4][256];
  __shared__ float gcol[128], wd_col[128];
  __shared__ int32_t t_sh, last_sh;
  const int tid = threadIdx.x;
  if (blk >= h.n1b + h.nb2) return;
  if (tid == 0) t_sh = atomicAdd(h.fin.iter, 0) + 1;
  if (blk < h.n1b) {
    tail_fold1_column_block<false>(h.j1, h.fo, h.w1t, blk, nullptr, &red[0][0], fred, gcol, wd_col, &t_sh, h.lr, h.beta1, h.beta2, h.eps);
    if (h.nb2 == 0) return;                     // (no finalize in this launch: the counter stays)
  } else {
    tail_reduce_adam(h.j2, blk - h.n1b, red, &t_sh, h.lr, h.beta1, h.beta2, h.eps);
  }
  __syncthreads();
  if (tid == 0) {
    // (No __threadfence() in front of the add.  The finalize reads NOTHING a job block of this launch wrote - the loss partials
    //  are an earlier launch's, the ring position only it writes - it only needs every job block to have READ the counter: a
    //  returned atomic, and the add's address depends on the value it returned, as in tail_check_in.  A change that makes the
    //  finalize read an output of a job needs a release here and an acquire in the finalize block.  The fence writes back an L2
    //  the sweep keeps dirty: spmm2_t 64.6 us with every thread fencing, 56.9 with thread 0 alone, 53.1 without -
    //  profiles/tail_hosted_ab.txt)
    int32_t t = t_sh;
    asm volatile("" : "+v"(t));
    last_sh = atomicAdd(h.fin.arrive + (t < 1 ? 1 : 0), 1) == h.n1b + h.nb2 - 1;
  }
  __syncthreads();
  if (!last_sh) return;
  tail_finalize_sums(h.fin, fred);
  if (tid == 0) {
    *h.fin.arrive = 0;
    *h.fin.pos = (*h.fin.pos + 1) % h.fin.capacity;
    atomicAdd(h.fin.iter, 1);
  }
}

}  // namespace gd
