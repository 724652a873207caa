// bn_act.hip — training-mode BatchNorm + activation, forward and backward, over NHWC bf16 matrices
// [M = N*H*W][C] with row pitch ld. All kernels are HBM-bound streaming passes: 16-B vector
// accesses along the channel axis, fp32 math, two-stage deterministic column reductions.
//
// Replaces aten::native_batch_norm(_backward) + aten::silu_/relu_ (+ residual add) reached from
// reference src/models/bricks/conv_module.py:211-213 and src/models/modules/yolo_modules.py:102.
#include <stdlib.h>
#include <type_traits>
#include "common.h"

namespace cvhip {

constexpr int kRedBlocksMax = 1024;
constexpr int kRedRowsPerBlockMin = 64;

static inline int colreduce_rows_host(int64_t M, int32_t C) {
  (void)C;
  const int min_rows = kRedRowsPerBlockMin;
  int64_t b = cdiv64(M, min_rows);
  if (b > kRedBlocksMax) b = kRedBlocksMax;
  if (b < 1) b = 1;
  return (int)b;
}

// MODE 0: (sum x, sum x^2)          MODE 1: (sum du, sum du*xhat)       MODE 2: (sum x, -)
// MODE 3 (round 5): the residual TAIL z = act(bn(y) + identity) of a ResNet bottleneck (torchvision Bottleneck.forward, reached through
// src/models/backbones/seg/resnet.py:91-94): du = dz * act'(z) from the saved OUTPUT z is computed, STORED (the identity branch's
// gradient) and reduced to the BatchNorm-backward sums (sum du, sum du*xhat) in ONE pass — read dz, read z, read y, write du — instead
// of an apply pass (read dz, read z, write du) followed by a reduction pass (read du, read y)
struct RedParams {
  const h16_t* a;   // x (mode 0/2) or dz (mode 1/3)
  const h16_t* y;   // conv output (mode 1/3)
  const h16_t* z;   // mode 3: the layer's saved output
  h16_t* du;        // mode 3: dz * act'(z), stored
  int ld_z, ld_du;
  int ld_a, ld_y;
  int64_t M;
  int C;
  const float *scale, *shift, *mean, *invstd;
  int act;
  float ap;
  float* partial;  // [gridDim.x][2][C]
  double* acc;     // or: fp64 accumulator [kAccShards][2][acc_ld] (atomics; common.h acc_add2) — no partial rows, no finalize launch
  int acc_ld;
  int addr32;      // a block's rows times the pitch fit 31 bits for every operand: 32-bit lane offsets (set by red_launch_dims)
};

// ACT: compile-time activation id for MODE 1 (a runtime switch inside the element loop compiles to a chain of scalar
// branches per element)
// A32: the lanes address the operands with 32-bit byte offsets from block-uniform bases (RedParams::addr32 holds); a kernel of its own
// rather than a branch, so that each form is register-allocated alone
template <int MODE, int ACT = 0, bool A32 = true>
__global__ __launch_bounds__(256) void colreduce_kernel(const RedParams p) {
  __shared__ float red[256 * 16];
  const int t = threadIdx.x;
  const int CV = (p.C + 7) >> 3;  // 16-B column vectors (C % 8 == 0 on the fast path)
  const bool vec = (p.C & 7) == 0 && (p.ld_a & 7) == 0 && ((MODE != 1 && MODE != 3) || (p.ld_y & 7) == 0) &&
                   (MODE != 3 || ((p.ld_z & 7) == 0 && (p.ld_du & 7) == 0 && (((uintptr_t)p.z | (uintptr_t)p.du) & 15) == 0)) &&
                   (((uintptr_t)p.a | (uintptr_t)p.y) & 15) == 0;
  const int cols_per_pass = CV < 256 ? CV : 256;
  const int rows_per_pass = 256 / cols_per_pass;
  const int tx = t % cols_per_pass, ty = t / cols_per_pass;
  const bool active = ty < rows_per_pass;
  const int64_t rows_per_block = cdiv64(p.M, gridDim.x);
  const int64_t r_begin = (int64_t)blockIdx.x * rows_per_block;
  int64_t r_end = r_begin + rows_per_block;
  if (r_end > p.M) r_end = p.M;

  for (int cv0 = 0; cv0 < CV; cv0 += cols_per_pass) {
    const int cv = cv0 + tx;
    f32x2 s1[4], s2[4];  // 8 channels as 4 pairs (common.h, pair-wise forms)
#pragma unroll
    for (int k = 0; k < 4; ++k) s1[k] = s2[k] = f32x2{0.f, 0.f};
    float sc[8], sh[8], mu[8], is[8];
    fill8c(1.f, sc);
    fill8c(0.f, sh);
    fill8c(0.f, mu);
    fill8c(1.f, is);
    if (MODE == 1 || MODE == 3) {
      const int cc = (cv < CV ? cv : CV - 1) * 8;
      if (p.scale) {  // uniform: scale/shift come together, mean/invstd come together
        load8c(p.scale, cc, p.C, sc);
        load8c(p.shift, cc, p.C, sh);
      }
      if (p.mean) {
        load8c(p.mean, cc, p.C, mu);
        load8c(p.invstd, cc, p.C, is);
      }
    }
    if (active && cv < CV) {
      // element-wise form: MODE 0 / 2, and every mode on the scalar path
      auto accum = [&](const f32x8& a, const f32x8& y) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float t1 = s1[j >> 1][j & 1], t2 = s2[j >> 1][j & 1];
          if (MODE == 0) {
            t1 += a.v[j];
            t2 += a.v[j] * a.v[j];
          } else if (MODE == 2) {
            t1 += a.v[j];
          } else if (MODE == 3) {
            // a = du (already masked and rounded to 16 bits by the caller below): the BatchNorm branch has no activation of its own
            const float xh = (y.v[j] - mu[j]) * is[j];
            t1 += a.v[j];
            t2 += a.v[j] * xh;
          } else {
            const float u = y.v[j] * sc[j] + sh[j];
            const float du = a.v[j] * act_bwd(u, ACT, p.ap);
            const float xh = (y.v[j] - mu[j]) * is[j];
            t1 += du;
            t2 += du * xh;
          }
          s1[j >> 1][j & 1] = t1;
          s2[j >> 1][j & 1] = t2;
        }
      };
      // 4 rows per trip: 4-8 independent 16-B loads in flight per lane before any arithmetic (HBM latency hiding). The LAST trip
      // of a block is the same code with its missing rows masked (clamped address, zero contribution): a remainder walked one
      // row per iteration cost up to 3 extra dependent memory round trips per block — on the 26 MB layers (100 rows per block,
      // one 64-row trip + 36 rows of remainder) more than the trip itself (2.4 TB/s against 3.8 for the aligned shapes).
      // (Software-pipelining the trips — next trip's loads issued before this trip's arithmetic — was measured in round 3: +32
      // VGPRs, no gain on the backward passes: they are co-limited by the quarter-rate v_exp_f32 / v_rcp_f32 of the SiLU derivative.)
      //
      // Addresses: the operand bases are block-uniform (advanced to the block's first row), a lane keeps one byte offset per operand
      // relative to them and adds a loop-invariant stride per trip. OFF is uint32_t when the host found that a block's rows times the
      // pitch fit 31 bits for every operand (RedParams::addr32; the loads then take the scalar-base + 32-bit-offset form and no trip
      // does 64-bit multiplies or adds in the VALU), int64_t otherwise.
      auto trips = [&]() {
        using OFF = std::conditional_t<A32, uint32_t, int64_t>;
        const int64_t left = r_end - r_begin;
        const OFF nr = (OFF)(left > 0 ? left : 0);
        const OFF stp = (OFF)rows_per_pass;
        const char* ab = reinterpret_cast<const char*>(p.a + r_begin * p.ld_a);
        const char* yb = reinterpret_cast<const char*>(p.y + ((MODE == 1 || MODE == 3) ? r_begin * p.ld_y : 0));
        const char* zb = reinterpret_cast<const char*>(p.z + (MODE == 3 ? r_begin * p.ld_z : 0));
        char* db = reinterpret_cast<char*>(p.du + (MODE == 3 ? r_begin * p.ld_du : 0));
        const OFF da = stp * (OFF)p.ld_a * 2, dy = stp * (OFF)p.ld_y * 2, dzs = stp * (OFF)p.ld_z * 2, dd = stp * (OFF)p.ld_du * 2;
        OFF oa = ((OFF)ty * (OFF)p.ld_a + (OFF)cv * 8) * 2, oy = ((OFF)ty * (OFF)p.ld_y + (OFF)cv * 8) * 2;
        OFF oz = ((OFF)ty * (OFF)p.ld_z + (OFF)cv * 8) * 2, od = ((OFF)ty * (OFF)p.ld_du + (OFF)cv * 8) * 2;
        f32x2 sc2[4], sh2[4], mu2[4], is2[4];
        pairs_of(sc, sc2);
        pairs_of(sh, sh2);
        pairs_of(mu, mu2);
        pairs_of(is, is2);
        for (OFF rr = (OFF)ty; rr < nr; rr += 4 * stp) {
          uint4 ua[4], uy[4], uz[MODE == 3 ? 4 : 1];
          bool ok[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            ok[q] = rr + (OFF)q * stp < nr;
            if constexpr (A32) {
              ua[q] = *reinterpret_cast<const uint4*>(ab + (ok[q] ? oa + (OFF)q * da : oa));
              if (MODE == 1 || MODE == 3) uy[q] = *reinterpret_cast<const uint4*>(yb + (ok[q] ? oy + (OFF)q * dy : oy));
              if constexpr (MODE == 3) uz[q] = *reinterpret_cast<const uint4*>(zb + (ok[q] ? oz + (OFF)q * dzs : oz));
            } else {  // 64-bit: the row's address from its index, every trip
              const int64_t rc = r_begin + (ok[q] ? rr + (OFF)q * stp : rr);
              ua[q] = *reinterpret_cast<const uint4*>(p.a + rc * p.ld_a + cv * 8);
              if (MODE == 1 || MODE == 3) uy[q] = *reinterpret_cast<const uint4*>(p.y + rc * p.ld_y + cv * 8);
              if constexpr (MODE == 3) uz[q] = *reinterpret_cast<const uint4*>(p.z + rc * p.ld_z + cv * 8);
            }
          }
          // every load of the trip is issued before any arithmetic: without the fence hipcc's scheduler sinks the loads of rows
          // 1..3 below the arithmetic of row 0 (fewer live registers) and waits vmcnt(0) after each — one row in flight per lane
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            // (round 6) a row slot that is past the block's last row for EVERY lane of the wave contributes nothing: its arithmetic —
            // the SiLU derivative is ~40 VALU instructions per element, and with 1024 blocks the mid-size layers run 1.56 / 3.125
            // trips per lane, i.e. up to 22 % masked slots — is skipped under a wave-uniform branch. Adding +0 changed no sum before.
            if (__builtin_amdgcn_ballot_w64(ok[q]) == 0) continue;
            if (!ok[q]) ua[q] = make_uint4(0u, 0u, 0u, 0u);  // x = 0 / dz = 0: no contribution to either sum (one select on the packed words)
            if constexpr (MODE == 3) {
              // du = dz * act'(z), rounded to 16 bits (what the stand-alone apply pass stores and the reduction pass then reads)
              f32x2 d[4], zz[4], yy[4];
              unpack_pairs(ua[q], d);
              unpack_pairs(uz[q], zz);
              unpack_pairs(uy[q], yy);
#pragma unroll
              for (int k = 0; k < 4; ++k) d[k] = d[k] * act_bwd2<ACT>(zz[k], p.ap);
              const uint4 packed = pack_pairs(d);
              if (ok[q]) {
                if constexpr (A32) *reinterpret_cast<uint4*>(db + (od + (OFF)q * dd)) = packed;
                else *reinterpret_cast<uint4*>(p.du + (r_begin + rr + (OFF)q * stp) * p.ld_du + cv * 8) = packed;
              }
              unpack_pairs(packed, d);
#pragma unroll
              for (int k = 0; k < 4; ++k) bn_bwd_sums2(d[k], yy[k], mu2[k], is2[k], s1[k], s2[k]);
            } else if constexpr (MODE == 1) {
              f32x2 d[4], yy[4];
              unpack_pairs(ua[q], d);
              unpack_pairs(uy[q], yy);
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                // the first row of a trip has always added the rounded du of the sigmoid-based activations to s1 and rows 1..3 the
                // fused product (what the optimizer made of the element-wise source); kept, so that the sums stay bit-identical
                if (q == 0 && (ACT == CVHIP_ACT_SILU || ACT == CVHIP_ACT_SIGMOID)) bnact_bwd_sums2<ACT, false>(d[k], yy[k], sc2[k], sh2[k], mu2[k], is2[k], p.ap, s1[k], s2[k]);
                else bnact_bwd_sums2<ACT, true>(d[k], yy[k], sc2[k], sh2[k], mu2[k], is2[k], p.ap, s1[k], s2[k]);
              }
            } else {
              accum(unpack8(ua[q]), f32x8{});
            }
          }
          if constexpr (A32) {
            oa += 4 * da;
            if (MODE == 1 || MODE == 3) oy += 4 * dy;
            if constexpr (MODE == 3) {
              oz += 4 * dzs;
              od += 4 * dd;
            }
          }
        }
      };
      if (vec) {
        trips();
      } else {
        for (int64_t r = r_begin + ty; r < r_end; r += rows_per_pass) {  // scalar path
          f32x8 a, y;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int c = cv * 8 + j;
            a.v[j] = c < p.C ? (float)p.a[r * p.ld_a + c] : 0.f;
            if (MODE == 1 || MODE == 3) y.v[j] = c < p.C ? (float)p.y[r * p.ld_y + c] : 0.f;
            if constexpr (MODE == 3) {
              if (c < p.C) {
                const h16_t dq = (h16_t)(a.v[j] * act_bwd((float)p.z[r * p.ld_z + c], ACT, p.ap));
                p.du[r * p.ld_du + c] = dq;
                a.v[j] = (float)dq;
              }
            }
          }
          accum(a, y);
        }
      }
    }
    // reduce over ty through LDS
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[t * 16 + j] = s1[j >> 1][j & 1];
      red[t * 16 + 8 + j] = s2[j >> 1][j & 1];
    }
    __syncthreads();
    // thread (tx, j16) sums over ty
    for (int idx = t; idx < cols_per_pass * 16; idx += 256) {
      const int x = idx >> 4, j = idx & 15;
      float s = 0.f;
      for (int yy = 0; yy < rows_per_pass; ++yy) s += red[(yy * cols_per_pass + x) * 16 + j];
      const int c = (cv0 + x) * 8 + (j & 7);
      if (cv0 + x < CV && c < p.C) {
        if (p.acc) unsafeAtomicAdd(p.acc + ((size_t)((blockIdx.x & (kAccShards - 1)) * 2 + (j >> 3))) * p.acc_ld + c, (double)s);
        else p.partial[((int64_t)blockIdx.x * 2 + (j >> 3)) * p.C + c] = s;
      }
    }
  }
}

// ---- partial-row pre-reduction -------------------------------------------------------------------
// The conv epilogue emits one partial row per M tile (25,600 rows for the YOLOv5-s stem at batch 64) and
// the streaming reductions up to 1024: reducing those serially in a one-thread-per-channel finalize
// kernel costs hundreds of microseconds of pure latency. When rows > kStage2Rows a fully parallel
// pre-pass folds them into kStage2Rows rows first, written to the scratch rows that every partial
// buffer carries behind its payload (CVHIP_REDUCE_SCRATCH_ROWS). Deterministic (fixed partition).
constexpr int kStage2Rows = CVHIP_REDUCE_SCRATCH_ROWS;
constexpr int kDirectRows = 1024;  // up to here the 64-lane finalize kernels read the partial rows themselves

__global__ __launch_bounds__(256) void rows_reduce_kernel(const float* __restrict__ in, int rows, int Wd, float* __restrict__ out) {
  __shared__ float red[4][64];
  const int t = threadIdx.x;
  const int col = blockIdx.x * 64 + (t & 63), lane = t >> 6;
  const int chunk = (rows + gridDim.y - 1) / gridDim.y;
  const int r0 = blockIdx.y * chunk;
  const int r1 = min(rows, r0 + chunk);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (col < Wd) {
    int r = r0 + lane;
    for (; r + 12 < r1; r += 16) {
      a0 += in[(int64_t)r * Wd + col];
      a1 += in[(int64_t)(r + 4) * Wd + col];
      a2 += in[(int64_t)(r + 8) * Wd + col];
      a3 += in[(int64_t)(r + 12) * Wd + col];
    }
    for (; r < r1; r += 4) a0 += in[(int64_t)r * Wd + col];
  }
  red[lane][t & 63] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (lane == 0 && col < Wd) out[(int64_t)blockIdx.y * Wd + col] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}

// returns the (possibly pre-reduced) partial pointer and updates *rows
static int direct_rows() { return kDirectRows; }

static const float* prereduce(const float* partial, int* rows, int Wd, hipStream_t s) {
  if (*rows <= direct_rows()) return partial;  // few enough rows for the 16-lane finalize kernels (4 independent chains per lane)
  float* scratch = const_cast<float*>(partial) + (int64_t)(*rows) * Wd;
  hipLaunchKernelGGL(rows_reduce_kernel, dim3(cdiv(Wd, 64), kStage2Rows), dim3(256), 0, s, partial, *rows, Wd, scratch);
  *rows = kStage2Rows;
  return scratch;
}

// ---- finalize kernels (one thread per channel) -----------------------------------------------------
// 256 threads = CPB channels x LPC row-lanes (LPC = 16: CPB = 16, for <= 64 partial rows; LPC = 64: CPB = 4, for up to
// kDirectRows rows — every lane then sums <= 16 rows with independent loads, i.e. ~2 L2 round trips instead of a
// rows_reduce_kernel launch + a finalize launch). The lanes of a channel are folded through LDS.
template <int LPC>
__device__ __forceinline__ void foldN(const float* partial, int rows, int C, int c, int lane, double* s1, double* s2, bool want2,
                                      double (*red)[LPC][256 / LPC + 1]) {
  double a = 0.0, b = 0.0;
  if (c < C) {
    // 4 independent accumulation chains: the loads of a lane are independent, only the adds chain
    double a1 = 0.0, a2 = 0.0, a3 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
    int r = lane;
    for (; r + 3 * LPC < rows; r += 4 * LPC) {
      a += (double)partial[((int64_t)r * 2 + 0) * C + c];
      a1 += (double)partial[((int64_t)(r + LPC) * 2 + 0) * C + c];
      a2 += (double)partial[((int64_t)(r + 2 * LPC) * 2 + 0) * C + c];
      a3 += (double)partial[((int64_t)(r + 3 * LPC) * 2 + 0) * C + c];
      if (want2) {
        b += (double)partial[((int64_t)r * 2 + 1) * C + c];
        b1 += (double)partial[((int64_t)(r + LPC) * 2 + 1) * C + c];
        b2 += (double)partial[((int64_t)(r + 2 * LPC) * 2 + 1) * C + c];
        b3 += (double)partial[((int64_t)(r + 3 * LPC) * 2 + 1) * C + c];
      }
    }
    for (; r < rows; r += LPC) {
      a += (double)partial[((int64_t)r * 2 + 0) * C + c];
      if (want2) b += (double)partial[((int64_t)r * 2 + 1) * C + c];
    }
    a = (a + a1) + (a2 + a3);
    b = (b + b1) + (b2 + b3);
  }
  constexpr int CPB = 256 / LPC;
  const int cc = threadIdx.x % CPB;
  red[0][lane][cc] = a;
  red[1][lane][cc] = b;
  __syncthreads();
  a = 0.0;
  b = 0.0;
  if (lane == 0) {
#pragma unroll 16
    for (int l = 0; l < LPC; ++l) {
      a += red[0][l][cc];
      b += red[1][l][cc];
    }
  }
  *s1 = a;
  *s2 = b;
}

template <int LPC>
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* partial, int rows, int C, double count, const float* gamma,
                                                          const float* beta, float* rmean, float* rvar, float momentum, float eps,
                                                          float* mean, float* invstd, float* scale, float* shift) {
  constexpr int CPB = 256 / LPC;
  __shared__ double red[2][LPC][CPB + 1];
  const int c = blockIdx.x * CPB + (threadIdx.x % CPB), lane = threadIdx.x / CPB;
  double s1, s2;
  foldN<LPC>(partial, rows, C, c, lane, &s1, &s2, true, red);
  if (lane != 0 || c >= C) return;
  const double m = s1 / count;
  double var = s2 / count - m * m;
  if (var < 0.0) var = 0.0;
  const float is = (float)(1.0 / sqrt(var + (double)eps));
  const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
  if (mean) mean[c] = (float)m;
  if (invstd) invstd[c] = is;
  const float sc = g * is;
  if (scale) scale[c] = sc;
  if (shift) shift[c] = b - (float)m * sc;
  if (rmean) rmean[c] = (1.f - momentum) * rmean[c] + momentum * (float)m;
  if (rvar) {
    const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
    rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)unb;
  }
}

__global__ void bn_eval_kernel(int C, const float* gamma, const float* beta, const float* rmean, const float* rvar,
                               float eps, float* scale, float* shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float is = 1.f / sqrtf(rvar[c] + eps);
  const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
  scale[c] = g * is;
  shift[c] = b - rmean[c] * g * is;
}

// out0[c] = sum_r partial[r][0][c]; out1[c] = sum_r partial[r][1][c]; optionally acc0/acc1 += the same sums
// (accumulate != 0 makes out0/out1 accumulate as well)
template <int LPC>
__global__ __launch_bounds__(256) void sum_partials_kernel(const float* partial, int rows, int C, float* out0, float* out1, int accumulate,
                                                           float* acc0, float* acc1) {
  constexpr int CPB = 256 / LPC;
  __shared__ double red[2][LPC][CPB + 1];
  const int c = blockIdx.x * CPB + (threadIdx.x % CPB), lane = threadIdx.x / CPB;
  double s1, s2;
  foldN<LPC>(partial, rows, C, c, lane, &s1, &s2, out1 != nullptr || acc1 != nullptr, red);
  if (lane != 0 || c >= C) return;
  if (out0) out0[c] = accumulate ? out0[c] + (float)s1 : (float)s1;
  if (out1) out1[c] = accumulate ? out1[c] + (float)s2 : (float)s2;
  if (acc0) acc0[c] += (float)s1;
  if (acc1) acc1[c] += (float)s2;
}

// ---- elementwise passes -----------------------------------------------------------------------------
struct EwParams {
  const h16_t *a, *y, *res;
  h16_t* out;
  int ld_a, ld_y, ld_res, ld_out;
  int64_t M;
  int C;
  const float *scale, *shift, *mean, *invstd, *dgamma, *dbeta;
  int act;
  float ap;
  float inv_count;
  int res_pre;  // MODE 0: residual is added BEFORE the activation (ResNet bottleneck: relu(bn(y) + identity))
  // ACC variants: the per-channel constants are derived in the block's prologue from an fp64 accumulator (common.h acc_fold2)
  // instead of being read from arrays a finalize launch prepared
  const double* acc;   // [kAccShards][2][acc_ld]: MODE 0 (sum y, sum y^2); MODE 1 (sum du, sum du*xhat)
  int acc_ld;
  double count;        // MODE 0: elements per channel
  const float *gamma, *beta;
  float *rmean, *rvar;
  float momentum, eps;
  float *o_mean, *o_invstd, *o_scale, *o_shift;   // MODE 0: block 0 stores the layer's statistics for backward
  float *o_dgamma, *o_dbeta;                       // MODE 1: block 0 stores (accumulate != 0: adds) the parameter gradients
  int accumulate;
  // RLZ instances (round 5, lazy activations): `res` is the RAW convolution output of the layer that produced the residual; the
  // pass applies that layer's BatchNorm scale / shift and the (same) activation to it on load: out = act(a*sc+sh) + act(res*rsc+rsh)
  const float *res_scale, *res_shift;
  int addr32;  // a block's rows times the pitch fit 31 bits for every operand: 32-bit lane offsets (set by ew_set_addr32)
};
constexpr int kEwAccMaxC = 2048;

// rows a lane loads per trip (all issued before the trip's arithmetic). Round 4: 8 rows for the one-tensor forms (-DCVHIP_EW_RPT0=8)
// measured neutral in the step (14.17-14.20 vs 14.08-14.16 ms) and on rotating tensors (profiles/r04_ew_grid_ab.log): the passes
// are not short of bytes in flight, and more, shorter blocks (CVHIP_EW_ROWS=4/8) LOSE 0.1-0.6 ms to the per-block prologue
// (requesting the first trip's rows AHEAD of the accumulator fold of the ACC forms was built too: 122 -> 186 VGPRs, 14.25 vs 14.07-14.18 ms: no gain)
#ifndef CVHIP_EW_RPT0
#define CVHIP_EW_RPT0 4
#endif
template <int MODE, bool HAS_RES>
struct EW_RPT {
  static constexpr int value = (MODE == 1 || HAS_RES || MODE == 3) ? 4 : CVHIP_EW_RPT0;
};

// MODE 0: out = act(a*scale+shift) (+res)         [a = conv output y]
// MODE 1: out = dy from (a = dz, y)               [BN+act backward apply]
// MODE 2: out = a (copy)       MODE 3: out = a + res
// RLZ (MODE 0 only): the residual operand is a LAZY activation — see EwParams::res_scale
// A32: as for colreduce_kernel (EwParams::addr32)
template <int MODE, int ACT = 0, bool ACC = false, bool RLZ = false, bool A32 = true>
__global__ __launch_bounds__(256) void ew_kernel(const EwParams p) {
  static_assert(!RLZ || MODE == 0, "lazy residuals exist in the forward apply pass only");
  __shared__ float cst[ACC ? 2 * kEwAccMaxC : 1];  // ACC: MODE 0 scale | shift; MODE 1 dbeta/M | dgamma/M
  if constexpr (ACC) {
    for (int c = threadIdx.x; c < p.C; c += 256) {
      double s1, s2;
      acc_fold2(p.acc, p.acc_ld, c, s1, s2);
      if (MODE == 0) {
        const double m = s1 / p.count;
        double var = s2 / p.count - m * m;
        if (var < 0.0) var = 0.0;
        const float is = (float)(1.0 / sqrt(var + (double)p.eps));
        const float g = p.gamma ? p.gamma[c] : 1.f, b = p.beta ? p.beta[c] : 0.f;
        const float sc = g * is, sh = b - (float)m * sc;
        cst[c] = sc;
        cst[kEwAccMaxC + c] = sh;
        if (blockIdx.x == 0) {  // the same arithmetic as bn_finalize_kernel
          p.o_mean[c] = (float)m;
          p.o_invstd[c] = is;
          p.o_scale[c] = sc;
          p.o_shift[c] = sh;
          if (p.rmean) p.rmean[c] = (1.f - p.momentum) * p.rmean[c] + p.momentum * (float)m;
          if (p.rvar) {
            const double unb = p.count > 1.0 ? var * p.count / (p.count - 1.0) : var;
            p.rvar[c] = (1.f - p.momentum) * p.rvar[c] + p.momentum * (float)unb;
          }
        }
      } else {
        cst[c] = (float)s1 * p.inv_count;                 // dbeta / M
        cst[kEwAccMaxC + c] = (float)s2 * p.inv_count;    // dgamma / M
        if (blockIdx.x == 0) {
          if (p.o_dbeta) p.o_dbeta[c] = p.accumulate ? p.o_dbeta[c] + (float)s1 : (float)s1;
          if (p.o_dgamma) p.o_dgamma[c] = p.accumulate ? p.o_dgamma[c] + (float)s2 : (float)s2;
        }
      }
    }
    __syncthreads();
  }
  const int CV = (p.C + 7) >> 3;
  const bool vec = (p.C & 7) == 0 && (p.ld_a & 7) == 0 && (p.ld_out & 7) == 0 &&
                   (MODE != 1 || (p.ld_y & 7) == 0) && (!p.res || (p.ld_res & 7) == 0) &&
                   (((uintptr_t)p.a | (uintptr_t)p.y | (uintptr_t)p.res | (uintptr_t)p.out) & 15) == 0;
  // thread owns one 16-B channel vector (tx) and walks rows: per-channel constants live in registers
  const int t = threadIdx.x;
  const int cols_per_pass = CV < 256 ? CV : 256;
  const int rows_per_pass = 256 / cols_per_pass;
  const int tx = t % cols_per_pass, ty = t / cols_per_pass;
  if (ty >= rows_per_pass) return;
  const int64_t rows_per_block = cdiv64(p.M, gridDim.x);
  const int64_t r_begin = (int64_t)blockIdx.x * rows_per_block;
  int64_t r_end = r_begin + rows_per_block;
  if (r_end > p.M) r_end = p.M;

  for (int cv = tx; cv < CV; cv += cols_per_pass) {
    const int c = cv * 8;
    float sc[8], sh[8], mu[8], is[8], k1[8], k2[8];
    fill8c(1.f, sc);
    fill8c(0.f, sh);
    fill8c(0.f, mu);
    fill8c(1.f, is);
    fill8c(0.f, k1);
    fill8c(0.f, k2);
    if (ACC && MODE == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int cc = c + j < p.C ? c + j : p.C - 1;
        sc[j] = cst[cc];
        sh[j] = cst[kEwAccMaxC + cc];
      }
    } else if (p.scale) {  // uniform branches: (scale, shift) and (mean, invstd, dgamma, dbeta) come as groups
      load8c(p.scale, c, p.C, sc);
      load8c(p.shift, c, p.C, sh);
    }
    if (MODE == 1 && p.mean) {
      load8c(p.mean, c, p.C, mu);
      load8c(p.invstd, c, p.C, is);
      if (ACC) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int cc = c + j < p.C ? c + j : p.C - 1;
          k1[j] = cst[cc];
          k2[j] = cst[kEwAccMaxC + cc];
        }
      } else {
        load8c(p.dbeta, c, p.C, k1);
        load8c(p.dgamma, c, p.C, k2);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          k1[j] *= p.inv_count;
          k2[j] *= p.inv_count;
        }
      }
    }
    float rsc[RLZ ? 8 : 1], rsh[RLZ ? 8 : 1];
    if constexpr (RLZ) {
      load8c(p.res_scale, c, p.C, rsc);
      load8c(p.res_shift, c, p.C, rsh);
    }
    // the residual mode is block-uniform: one branch-free instance of the row loops per mode (with the runtime tests inside the
    // element loop hipcc emitted a branch per element and no packed fp32 math: ISA of ew_kernel<0, SILU>, round 3)
    auto rows = [&](auto rm) {
      constexpr int RES = decltype(rm)::value;  // 0: no residual, 1: added after the activation (MODE 3: the add itself), 2: before, 3: lazy, after
      auto math = [&](const f32x8& a, const f32x8& y, const f32x8& rs) -> f32x8 {
        f32x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (MODE == 0) {
            float u = a.v[j] * sc[j] + sh[j];
            if (RES == 2) u += rs.v[j];
            float v = act_fwd(u, ACT, p.ap);
            if (RES == 1) v += rs.v[j];
            if constexpr (RES == 3) v += (float)(h16_t)act_fwd(rs.v[j] * rsc[j] + rsh[j], ACT, p.ap);  // rounded as the stand-alone pass stores it
            o.v[j] = v;
          } else if (MODE == 1) {
            const float u = y.v[j] * sc[j] + sh[j];
            const float du = a.v[j] * act_bwd(u, ACT, p.ap);
            if (p.mean) {
              const float xh = (y.v[j] - mu[j]) * is[j];
              o.v[j] = sc[j] * (du - k1[j] - xh * k2[j]);
            } else {
              o.v[j] = sc[j] * du;
            }
          } else if (MODE == 2) {
            o.v[j] = a.v[j];
          } else {
            o.v[j] = a.v[j] + rs.v[j];
          }
        }
        return o;
      };
      constexpr bool has_res = RES != 0;
      // 4 rows per trip: all loads of the trip are issued before the arithmetic (bytes in flight per lane x4); the block's last
      // trip runs the same code with its missing rows masked (clamped loads, no store) instead of a row-at-a-time remainder.
      // Addresses as in colreduce_kernel: block-uniform bases, per-lane byte offsets of type OFF advanced by a loop-invariant stride.
      auto trips = [&](auto stats_tag) {
        using OFF = std::conditional_t<A32, uint32_t, int64_t>;
        constexpr bool STATS = decltype(stats_tag)::value;  // MODE 1: the batch-statistics terms are present (p.mean)
        const int64_t left = r_end - r_begin;
        const OFF nr = (OFF)(left > 0 ? left : 0);
        const OFF stp = (OFF)rows_per_pass;
        constexpr int RPT = EW_RPT<MODE, has_res>::value;
        const char* ab = reinterpret_cast<const char*>(p.a + r_begin * p.ld_a);
        const char* yb = reinterpret_cast<const char*>(p.y + (MODE == 1 ? r_begin * p.ld_y : 0));
        const char* rb = reinterpret_cast<const char*>(p.res + (has_res ? r_begin * p.ld_res : 0));
        char* ob = reinterpret_cast<char*>(p.out + r_begin * p.ld_out);
        const OFF da = stp * (OFF)p.ld_a * 2, dy = stp * (OFF)p.ld_y * 2, dr = stp * (OFF)p.ld_res * 2, dout = stp * (OFF)p.ld_out * 2;
        OFF oa = ((OFF)ty * (OFF)p.ld_a + (OFF)c) * 2, oy = ((OFF)ty * (OFF)p.ld_y + (OFF)c) * 2;
        OFF ores = ((OFF)ty * (OFF)p.ld_res + (OFF)c) * 2, oo = ((OFF)ty * (OFF)p.ld_out + (OFF)c) * 2;
        f32x2 sc2[4], sh2[4], mu2[4], is2[4], k12[4], k22[4], rsc2[4], rsh2[4];
        pairs_of(sc, sc2);
        pairs_of(sh, sh2);
        pairs_of(mu, mu2);
        pairs_of(is, is2);
        pairs_of(k1, k12);
        pairs_of(k2, k22);
        if constexpr (RLZ) {
          pairs_of(rsc, rsc2);
          pairs_of(rsh, rsh2);
        }
        for (OFF rr = (OFF)ty; rr < nr; rr += RPT * stp) {
          uint4 ua[RPT], uy[RPT], ur[RPT];
          bool ok[RPT];
#pragma unroll
          for (int q = 0; q < RPT; ++q) {
            ok[q] = rr + (OFF)q * stp < nr;
            if constexpr (A32) {
              ua[q] = *reinterpret_cast<const uint4*>(ab + (ok[q] ? oa + (OFF)q * da : oa));
              if (MODE == 1) uy[q] = *reinterpret_cast<const uint4*>(yb + (ok[q] ? oy + (OFF)q * dy : oy));
              if (has_res) ur[q] = *reinterpret_cast<const uint4*>(rb + (ok[q] ? ores + (OFF)q * dr : ores));
            } else {  // 64-bit: the row's address from its index, every trip
              const int64_t rc = r_begin + (ok[q] ? rr + (OFF)q * stp : rr);
              ua[q] = *reinterpret_cast<const uint4*>(p.a + rc * p.ld_a + c);
              if (MODE == 1) uy[q] = *reinterpret_cast<const uint4*>(p.y + rc * p.ld_y + c);
              if (has_res) ur[q] = *reinterpret_cast<const uint4*>(p.res + rc * p.ld_res + c);
            }
          }
          __builtin_amdgcn_sched_barrier(0);  // loads of all rows of the trip first (see colreduce_kernel)
#pragma unroll
          for (int q = 0; q < RPT; ++q) {
            uint4 packed;
            if constexpr (MODE == 0) {
              f32x2 a[4], rs[4], o[4];
              unpack_pairs(ua[q], a);
              if (has_res) unpack_pairs(ur[q], rs);
#pragma unroll
              for (int k = 0; k < 4; ++k) {
                f32x2 r2 = has_res ? rs[k] : f32x2{0.f, 0.f};
                if constexpr (RES == 3) {  // the lazy residual, rounded as the stand-alone pass stores it
                  const f32x2 v = act_fwd2<ACT, false>(fma2(rs[k], rsc2[k], rsh2[k]), p.ap, f32x2{0.f, 0.f});
                  r2 = unpack_pair(pack2(v.x, v.y));
                }
                o[k] = bnact_fwd2<ACT, RES == 3 ? 1 : RES>(a[k], sc2[k], sh2[k], r2, p.ap);
              }
              packed = pack_pairs(o);
            } else if constexpr (MODE == 1) {
              f32x2 d[4], yy[4], o[4];
              unpack_pairs(ua[q], d);
              unpack_pairs(uy[q], yy);
#pragma unroll
              for (int k = 0; k < 4; ++k) o[k] = bnact_bwd_apply2<ACT, STATS>(d[k], yy[k], sc2[k], sh2[k], mu2[k], is2[k], k12[k], k22[k], p.ap);
              packed = pack_pairs(o);
            } else {
              packed = pack8(math(unpack8(ua[q]), f32x8{}, has_res ? unpack8(ur[q]) : f32x8{}));
            }
            if (ok[q]) {
              if constexpr (A32) *reinterpret_cast<uint4*>(ob + (oo + (OFF)q * dout)) = packed;
              else *reinterpret_cast<uint4*>(p.out + (r_begin + rr + (OFF)q * stp) * p.ld_out + c) = packed;
            }
          }
          if constexpr (A32) {
            oa += RPT * da;
            if (MODE == 1) oy += RPT * dy;
            if (has_res) ores += RPT * dr;
            oo += RPT * dout;
          }
        }
      };
      if (vec) {
        bool stats = false;
        if constexpr (MODE == 1) stats = p.mean != nullptr;
        if constexpr (MODE == 1) {
          if (stats) trips(std::true_type{});
        }
        if (!stats) trips(std::false_type{});
      } else {
        for (int64_t r = r_begin + ty; r < r_end; r += rows_per_pass) {  // scalar path
          f32x8 a, y, rs;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const bool okc = c + j < p.C;
            a.v[j] = okc ? (float)p.a[r * p.ld_a + c + j] : 0.f;
            if (MODE == 1) y.v[j] = okc ? (float)p.y[r * p.ld_y + c + j] : 0.f;
            if (has_res) rs.v[j] = okc ? (float)p.res[r * p.ld_res + c + j] : 0.f;
          }
          const f32x8 o = math(a, y, rs);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (c + j < p.C) p.out[r * p.ld_out + c + j] = (h16_t)o.v[j];
        }
      }
    };
    if constexpr (RLZ) {
      rows(std::integral_constant<int, 3>{});
    } else if constexpr (MODE == 3) {
      rows(std::integral_constant<int, 1>{});
    } else if constexpr (MODE == 0) {
      if (!p.res) rows(std::integral_constant<int, 0>{});
      else if (p.res_pre) rows(std::integral_constant<int, 2>{});
      else rows(std::integral_constant<int, 1>{});
    } else {
      rows(std::integral_constant<int, 0>{});
    }
  }
}

// Round 5 (lazy activations): a layer whose BN + activation apply pass is deferred into its consumers' loads still needs its
// statistics finalized — mean | invstd | scale | shift for backward and for the consumers' prologues, running statistics updated.
// The same arithmetic as block 0 of ew_kernel<0, ACT, true>'s prologue, as a launch of its own (C / 256 blocks).
__global__ __launch_bounds__(256) void bn_finalize_acc_kernel(const double* acc, int acc_ld, int C, double count, const float* gamma,
                                                              const float* beta, float* rmean, float* rvar, float momentum, float eps,
                                                              float* o_mean, float* o_invstd, float* o_scale, float* o_shift) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s1, s2;
  acc_fold2(acc, acc_ld, c, s1, s2);
  const double m = s1 / count;
  double var = s2 / count - m * m;
  if (var < 0.0) var = 0.0;
  const float is = (float)(1.0 / sqrt(var + (double)eps));
  const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
  const float sc = g * is, sh = b - (float)m * sc;
  o_mean[c] = (float)m;
  o_invstd[c] = is;
  o_scale[c] = sc;
  o_shift[c] = sh;
  if (rmean) rmean[c] = (1.f - momentum) * rmean[c] + momentum * (float)m;
  if (rvar) {
    const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
    rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)unb;
  }
}

// blocks are row chunks; a thread moves 16 B per row visit, so ~32 row-visits per thread keeps
// enough bytes in flight while leaving >> 256 blocks for large activations
// launch KERNEL<MODE, act> for the runtime activation id
// launch the A32 or the 64-bit instance of a kernel, as the host found for this launch (PARAMS.addr32)
#define CVHIP_LAUNCH_A32(KERNEL, GRID, STREAM, PARAMS, ...)                                                     \
  do {                                                                                                          \
    if ((PARAMS).addr32) hipLaunchKernelGGL((KERNEL<__VA_ARGS__, true>), GRID, dim3(256), 0, STREAM, PARAMS);   \
    else hipLaunchKernelGGL((KERNEL<__VA_ARGS__, false>), GRID, dim3(256), 0, STREAM, PARAMS);                  \
  } while (0)

#define CVHIP_LAUNCH_ACT_ACC(KERNEL, MODE, ACTV, GRID, STREAM, PARAMS)                                              \
  switch (ACTV) {                                                                                                   \
    case CVHIP_ACT_RELU: CVHIP_LAUNCH_A32(KERNEL, GRID, STREAM, PARAMS, MODE, CVHIP_ACT_RELU, true, false); break;       \
    case CVHIP_ACT_SILU: CVHIP_LAUNCH_A32(KERNEL, GRID, STREAM, PARAMS, MODE, CVHIP_ACT_SILU, true, false); break;       \
    case CVHIP_ACT_LEAKY: CVHIP_LAUNCH_A32(KERNEL, GRID, STREAM, PARAMS, MODE, CVHIP_ACT_LEAKY, true, false); break;     \
    case CVHIP_ACT_SIGMOID: CVHIP_LAUNCH_A32(KERNEL, GRID, STREAM, PARAMS, MODE, CVHIP_ACT_SIGMOID, true, false); break; \
    case CVHIP_ACT_HSWISH: CVHIP_LAUNCH_A32(KERNEL, GRID, STREAM, PARAMS, MODE, CVHIP_ACT_HSWISH, true, false); break;   \
    default: CVHIP_LAUNCH_A32(KERNEL, GRID, STREAM, PARAMS, MODE, CVHIP_ACT_NONE, true, false); break;                  \
  }

// TAIL: the template arguments between the activation and A32 (ew_kernel: `false, false`; colreduce_kernel: none)
#define CVHIP_LAUNCH_ACT(KERNEL, MODE, ACTV, GRID, STREAM, PARAMS, ...)                                               \
  switch (ACTV) {                                                                                                     \
    case CVHIP_ACT_RELU: CVHIP_LAUNCH_A32(KERNEL, GRID, STREAM, PARAMS, MODE, CVHIP_ACT_RELU __VA_ARGS__); break;       \
    case CVHIP_ACT_SILU: CVHIP_LAUNCH_A32(KERNEL, GRID, STREAM, PARAMS, MODE, CVHIP_ACT_SILU __VA_ARGS__); break;       \
    case CVHIP_ACT_LEAKY: CVHIP_LAUNCH_A32(KERNEL, GRID, STREAM, PARAMS, MODE, CVHIP_ACT_LEAKY __VA_ARGS__); break;     \
    case CVHIP_ACT_SIGMOID: CVHIP_LAUNCH_A32(KERNEL, GRID, STREAM, PARAMS, MODE, CVHIP_ACT_SIGMOID __VA_ARGS__); break; \
    case CVHIP_ACT_HSWISH: CVHIP_LAUNCH_A32(KERNEL, GRID, STREAM, PARAMS, MODE, CVHIP_ACT_HSWISH __VA_ARGS__); break;   \
    default: CVHIP_LAUNCH_A32(KERNEL, GRID, STREAM, PARAMS, MODE, CVHIP_ACT_NONE __VA_ARGS__); break;                  \
  }
#define CVHIP_EW_PLAIN , false, false

static int ew_rows_per_thread() { return 16; }   // (4 / 8 rows per thread lose 0.1-0.6 ms per step to the per-block prologue: profiles/r04_ew_grid_ab.log)

// ((rows of a block) * pitch + C) 16-bit elements stay below 2^31 bytes: the lanes of a block can address the operand with 32-bit offsets
static inline bool fits31(int64_t rows, int ld, int C) { return (rows * (int64_t)ld + C) * 2 < ((int64_t)1 << 31); }

static inline int ew_grid(int64_t M, int C);
// the grid of an elementwise launch; sets p.addr32 for it
static inline dim3 ew_dims(EwParams& p) {
  const int grid = ew_grid(p.M, p.C);
  const int64_t rows = cdiv64(p.M, grid);
  p.addr32 = fits31(rows, p.ld_a, p.C) && fits31(rows, p.ld_out, p.C) && (!p.y || fits31(rows, p.ld_y, p.C)) &&
             (!p.res || fits31(rows, p.ld_res, p.C));
  return dim3(grid);
}
// the grid of a column-reduction launch; sets p.addr32 for it
static inline dim3 red_dims(RedParams& p) {
  const int grid = colreduce_rows_host(p.M, p.C);
  const int64_t rows = cdiv64(p.M, grid);
  p.addr32 = fits31(rows, p.ld_a, p.C) && (!p.y || fits31(rows, p.ld_y, p.C)) && (!p.z || fits31(rows, p.ld_z, p.C)) &&
             (!p.du || fits31(rows, p.ld_du, p.C));
  return dim3(grid);
}

static inline int ew_grid(int64_t M, int C) {
  const int CV = (C + 7) / 8;
  const int cols = CV < 256 ? CV : 256;
  const int rows_per_pass = 256 / cols;
  int64_t b = cdiv64(M, (int64_t)rows_per_pass * ew_rows_per_thread());
  if (b > 256 * 32) b = 256 * 32;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace cvhip

using namespace cvhip;

extern "C" {

int cvhip_colreduce_rows(int64_t M, int32_t C) { return colreduce_rows_host(M, C); }

static int launch_red(int mode, RedParams& p, hipStream_t s) {
  if (!p.a || !p.partial || p.M < 0 || p.C <= 0) return CVHIP_ERR_INVALID;
  const dim3 grid = red_dims(p);
  if (mode == 0) CVHIP_LAUNCH_A32(colreduce_kernel, grid, s, p, 0, 0);
  else if (mode == 1) {
    CVHIP_LAUNCH_ACT(colreduce_kernel, 1, p.act, grid, s, p)
  }
  else CVHIP_LAUNCH_A32(colreduce_kernel, grid, s, p, 2, 0);
  return check_launch("colreduce_kernel");
}

int cvhip_bn_stats_partial(const void* x, int64_t M, int32_t C, int32_t ld, float* partial, void* stream) {
  RedParams p{};
  p.a = (const h16_t*)x;
  p.ld_a = ld;
  p.M = M;
  p.C = C;
  p.partial = partial;
  return launch_red(0, p, (hipStream_t)stream);
}

int cvhip_colsum_partial(const void* x, int64_t M, int32_t C, int32_t ld, float* partial, void* stream) {
  RedParams p{};
  p.a = (const h16_t*)x;
  p.ld_a = ld;
  p.M = M;
  p.C = C;
  p.partial = partial;
  return launch_red(2, p, (hipStream_t)stream);
}

int cvhip_bn_act_bwd_partial(const void* dz, int32_t ld_dz, const void* y, int32_t ld_y, int64_t M, int32_t C,
                             const float* scale, const float* shift, const float* mean, const float* invstd,
                             int32_t act, float act_param, float* partial, void* stream) {
  if (!y) return CVHIP_ERR_INVALID;
  RedParams p{};
  p.a = (const h16_t*)dz;
  p.y = (const h16_t*)y;
  p.ld_a = ld_dz;
  p.ld_y = ld_y;
  p.M = M;
  p.C = C;
  p.scale = scale;
  p.shift = shift;
  p.mean = mean;
  p.invstd = invstd;
  p.act = act;
  p.ap = act_param;
  p.partial = partial;
  return launch_red(1, p, (hipStream_t)stream);
}

int cvhip_bn_finalize(const float* partial, int32_t rows, int32_t C, int64_t count, const float* gamma,
                      const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                      float* mean, float* invstd, float* scale, float* shift, void* stream) {
  if (!partial || rows <= 0 || C <= 0 || count <= 0) return CVHIP_ERR_INVALID;
  partial = prereduce(partial, &rows, 2 * C, (hipStream_t)stream);
  if (rows > kStage2Rows)
    hipLaunchKernelGGL(bn_finalize_kernel<64>, dim3(cdiv(C, 4)), dim3(256), 0, (hipStream_t)stream, partial, rows, C,
                       (double)count, gamma, beta, running_mean, running_var, momentum, eps, mean, invstd, scale, shift);
  else
    hipLaunchKernelGGL(bn_finalize_kernel<16>, dim3(cdiv(C, 16)), dim3(256), 0, (hipStream_t)stream, partial, rows, C,
                       (double)count, gamma, beta, running_mean, running_var, momentum, eps, mean, invstd, scale, shift);
  return check_launch("bn_finalize_kernel");
}

int cvhip_bn_eval_scale_shift(int32_t C, const float* gamma, const float* beta, const float* running_mean,
                              const float* running_var, float eps, float* scale, float* shift, void* stream) {
  if (C <= 0 || !running_mean || !running_var || !scale || !shift) return CVHIP_ERR_INVALID;
  hipLaunchKernelGGL(bn_eval_kernel, dim3(cdiv(C, 64)), dim3(64), 0, (hipStream_t)stream, C, gamma, beta,
                     running_mean, running_var, eps, scale, shift);
  return check_launch("bn_eval_kernel");
}

int cvhip_bn_bwd_finalize(const float* partial, int32_t rows, int32_t C, float* dgamma, float* dbeta, float* acc_dgamma,
                          float* acc_dbeta, void* stream) {
  if (!partial || rows <= 0 || C <= 0) return CVHIP_ERR_INVALID;
  partial = prereduce(partial, &rows, 2 * C, (hipStream_t)stream);
  if (rows > kStage2Rows)
    hipLaunchKernelGGL(sum_partials_kernel<64>, dim3(cdiv(C, 4)), dim3(256), 0, (hipStream_t)stream, partial, rows, C,
                       dbeta, dgamma, 0, acc_dbeta, acc_dgamma);
  else
    hipLaunchKernelGGL(sum_partials_kernel<16>, dim3(cdiv(C, 16)), dim3(256), 0, (hipStream_t)stream, partial, rows, C,
                       dbeta, dgamma, 0, acc_dbeta, acc_dgamma);
  return check_launch("sum_partials_kernel");
}

int cvhip_colsum_finalize(const float* partial, int32_t rows, int32_t C, float* out, int accumulate, void* stream) {
  if (!partial || rows <= 0 || C <= 0 || !out) return CVHIP_ERR_INVALID;
  partial = prereduce(partial, &rows, 2 * C, (hipStream_t)stream);
  if (rows > kStage2Rows)
    hipLaunchKernelGGL(sum_partials_kernel<64>, dim3(cdiv(C, 4)), dim3(256), 0, (hipStream_t)stream, partial, rows, C,
                       out, (float*)nullptr, accumulate, (float*)nullptr, (float*)nullptr);
  else
    hipLaunchKernelGGL(sum_partials_kernel<16>, dim3(cdiv(C, 16)), dim3(256), 0, (hipStream_t)stream, partial, rows, C,
                       out, (float*)nullptr, accumulate, (float*)nullptr, (float*)nullptr);
  return check_launch("sum_partials_kernel");
}

int cvhip_bn_act_fwd(const void* y, int32_t ld_y, void* z, int32_t ld_z, int64_t M, int32_t C, const float* scale,
                     const float* shift, int32_t act, float act_param, const void* residual, int32_t ld_res,
                     void* stream) {
  if (!y || !z || M < 0 || C <= 0) return CVHIP_ERR_INVALID;
  if (M == 0) return CVHIP_OK;
  EwParams p{};
  p.a = (const h16_t*)y;
  p.ld_a = ld_y;
  p.out = (h16_t*)z;
  p.ld_out = ld_z;
  p.res = (const h16_t*)residual;
  p.ld_res = ld_res;
  p.M = M;
  p.C = C;
  p.scale = scale;
  p.shift = shift;
  p.act = act;
  p.ap = act_param;
  const dim3 grid = ew_dims(p);
  CVHIP_LAUNCH_ACT(ew_kernel, 0, act, grid, (hipStream_t)stream, p, CVHIP_EW_PLAIN)
  return check_launch("ew_kernel<0>");
}

int cvhip_bn_add_act_fwd(const void* y, int32_t ld_y, void* z, int32_t ld_z, int64_t M, int32_t C, const float* scale,
                         const float* shift, int32_t act, float act_param, const void* residual, int32_t ld_res, void* stream) {
  if (!y || !z || !residual || M < 0 || C <= 0) return CVHIP_ERR_INVALID;
  if (M == 0) return CVHIP_OK;
  EwParams p{};
  p.a = (const h16_t*)y;
  p.ld_a = ld_y;
  p.out = (h16_t*)z;
  p.ld_out = ld_z;
  p.res = (const h16_t*)residual;
  p.ld_res = ld_res;
  p.M = M;
  p.C = C;
  p.scale = scale;
  p.shift = shift;
  p.act = act;
  p.ap = act_param;
  p.res_pre = 1;  // the residual joins BEFORE the activation
  const dim3 grid = ew_dims(p);
  CVHIP_LAUNCH_ACT(ew_kernel, 0, act, grid, (hipStream_t)stream, p, CVHIP_EW_PLAIN)
  return check_launch("ew_kernel<0>(bn_add_act)");
}

int cvhip_bn_act_bwd_apply(const void* dz, int32_t ld_dz, const void* y, int32_t ld_y, void* dy, int32_t ld_dy,
                           int64_t M, int32_t C, const float* scale, const float* shift, const float* mean,
                           const float* invstd, const float* dgamma, const float* dbeta, int32_t act,
                           float act_param, void* stream) {
  if (!dz || !y || !dy || M < 0 || C <= 0) return CVHIP_ERR_INVALID;
  if (mean && (!invstd || !dgamma || !dbeta)) return CVHIP_ERR_INVALID;
  if (M == 0) return CVHIP_OK;
  EwParams p{};
  p.a = (const h16_t*)dz;
  p.ld_a = ld_dz;
  p.y = (const h16_t*)y;
  p.ld_y = ld_y;
  p.out = (h16_t*)dy;
  p.ld_out = ld_dy;
  p.M = M;
  p.C = C;
  p.scale = scale;
  p.shift = shift;
  p.mean = mean;
  p.invstd = invstd;
  p.dgamma = dgamma;
  p.dbeta = dbeta;
  p.act = act;
  p.ap = act_param;
  p.inv_count = 1.f / (float)M;
  const dim3 grid = ew_dims(p);
  CVHIP_LAUNCH_ACT(ew_kernel, 1, act, grid, (hipStream_t)stream, p, CVHIP_EW_PLAIN)
  return check_launch("ew_kernel<1>");
}

int cvhip_add_act_fwd(const void* a, int32_t ld_a, const void* b, int32_t ld_b, void* out, int32_t ld_out, int64_t M, int32_t C,
                      int32_t act, float act_param, void* stream) {
  if (!a || !b || !out || M < 0 || C <= 0) return CVHIP_ERR_INVALID;
  if (M == 0) return CVHIP_OK;
  EwParams p{};
  p.a = (const h16_t*)a;
  p.ld_a = ld_a;
  p.res = (const h16_t*)b;
  p.ld_res = ld_b;
  p.out = (h16_t*)out;
  p.ld_out = ld_out;
  p.M = M;
  p.C = C;
  p.act = act;
  p.ap = act_param;
  p.res_pre = 1;
  const dim3 grid = ew_dims(p);
  CVHIP_LAUNCH_ACT(ew_kernel, 0, act, grid, (hipStream_t)stream, p, CVHIP_EW_PLAIN)
  return check_launch("ew_kernel<0>(add_act)");
}

int cvhip_copy2d(const void* src, int32_t ld_src, void* dst, int32_t ld_dst, int64_t M, int32_t C, void* stream) {
  if (!src || !dst || M < 0 || C <= 0) return CVHIP_ERR_INVALID;
  if (M == 0) return CVHIP_OK;
  EwParams p{};
  p.a = (const h16_t*)src;
  p.ld_a = ld_src;
  p.out = (h16_t*)dst;
  p.ld_out = ld_dst;
  p.M = M;
  p.C = C;
  const dim3 grid = ew_dims(p);
  CVHIP_LAUNCH_A32(ew_kernel, grid, (hipStream_t)stream, p, 2, 0, false, false);
  return check_launch("ew_kernel<2>");
}

int cvhip_add2d(const void* a, int32_t ld_a, const void* b, int32_t ld_b, void* dst, int32_t ld_dst, int64_t M,
                int32_t C, void* stream) {
  if (!a || !b || !dst || M < 0 || C <= 0) return CVHIP_ERR_INVALID;
  if (M == 0) return CVHIP_OK;
  EwParams p{};
  p.a = (const h16_t*)a;
  p.ld_a = ld_a;
  p.res = (const h16_t*)b;
  p.ld_res = ld_b;
  p.out = (h16_t*)dst;
  p.ld_out = ld_dst;
  p.M = M;
  p.C = C;
  const dim3 grid = ew_dims(p);
  CVHIP_LAUNCH_A32(ew_kernel, grid, (hipStream_t)stream, p, 3, 0, false, false);
  return check_launch("ew_kernel<3>");
}

int cvhip_bn_acc_shards(void) { return kAccShards; }

int cvhip_bn_act_bwd_sums_acc(const void* dz, int32_t ld_dz, const void* y, int32_t ld_y, int64_t M, int32_t C, const float* scale,
                              const float* shift, const float* mean, const float* invstd, int32_t act, float act_param, double* acc,
                              int32_t acc_ld, void* stream) {
  if (!dz || !y || !acc || M < 0 || C <= 0 || acc_ld < C) return CVHIP_ERR_INVALID;
  if (M == 0) return CVHIP_OK;
  RedParams p{};
  p.a = (const h16_t*)dz;
  p.y = (const h16_t*)y;
  p.ld_a = ld_dz;
  p.ld_y = ld_y;
  p.M = M;
  p.C = C;
  p.scale = scale;
  p.shift = shift;
  p.mean = mean;
  p.invstd = invstd;
  p.act = act;
  p.ap = act_param;
  p.acc = acc;
  p.acc_ld = acc_ld;
  const dim3 grid = red_dims(p);
  CVHIP_LAUNCH_ACT(colreduce_kernel, 1, act, grid, (hipStream_t)stream, p)
  return check_launch("colreduce_kernel(acc)");
}

int cvhip_bn_tail_bwd_sums_acc(const void* dz, int32_t ld_dz, const void* z_out, int32_t ld_z, const void* y, int32_t ld_y, void* du, int32_t ld_du,
                               int64_t M, int32_t C, const float* mean, const float* invstd, int32_t act, float act_param, double* acc,
                               int32_t acc_ld, void* stream) {
  if (!dz || !z_out || !y || !du || !mean || !invstd || !acc || M < 0 || C <= 0 || acc_ld < C) return CVHIP_ERR_INVALID;
  if (act != CVHIP_ACT_NONE && act != CVHIP_ACT_RELU && act != CVHIP_ACT_LEAKY) return CVHIP_ERR_UNSUPPORTED;  // act'(z) from the OUTPUT's sign
  if (M == 0) return CVHIP_OK;
  RedParams p{};
  p.a = (const h16_t*)dz;
  p.ld_a = ld_dz;
  p.y = (const h16_t*)y;
  p.ld_y = ld_y;
  p.z = (const h16_t*)z_out;
  p.ld_z = ld_z;
  p.du = (h16_t*)du;
  p.ld_du = ld_du;
  p.M = M;
  p.C = C;
  p.mean = mean;
  p.invstd = invstd;
  p.act = act;
  p.ap = act_param;
  p.acc = acc;
  p.acc_ld = acc_ld;
  const dim3 grid = red_dims(p);
  switch (act) {
    case CVHIP_ACT_RELU: CVHIP_LAUNCH_A32(colreduce_kernel, grid, (hipStream_t)stream, p, 3, CVHIP_ACT_RELU); break;
    case CVHIP_ACT_LEAKY: CVHIP_LAUNCH_A32(colreduce_kernel, grid, (hipStream_t)stream, p, 3, CVHIP_ACT_LEAKY); break;
    default: CVHIP_LAUNCH_A32(colreduce_kernel, grid, (hipStream_t)stream, p, 3, CVHIP_ACT_NONE); break;
  }
  return check_launch("colreduce_kernel<3>(acc)");
}

int cvhip_bn_act_fwd_acc(const void* y, int32_t ld_y, void* z, int32_t ld_z, int64_t M, int32_t C, const double* acc, int32_t acc_ld,
                         int64_t count, const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                         float eps, float* mean, float* invstd, float* scale, float* shift, int32_t act, float act_param,
                         const void* residual, int32_t ld_res, int32_t res_pre, void* stream) {
  if (!y || !z || !acc || !mean || !invstd || !scale || !shift || M <= 0 || C <= 0 || count <= 0 || acc_ld < C) return CVHIP_ERR_INVALID;
  if (C > kEwAccMaxC) return CVHIP_ERR_UNSUPPORTED;
  EwParams p{};
  p.a = (const h16_t*)y;
  p.ld_a = ld_y;
  p.out = (h16_t*)z;
  p.ld_out = ld_z;
  p.res = (const h16_t*)residual;
  p.ld_res = ld_res;
  p.res_pre = residual ? res_pre : 0;
  p.M = M;
  p.C = C;
  p.act = act;
  p.ap = act_param;
  p.acc = acc;
  p.acc_ld = acc_ld;
  p.count = (double)count;
  p.gamma = gamma;
  p.beta = beta;
  p.rmean = running_mean;
  p.rvar = running_var;
  p.momentum = momentum;
  p.eps = eps;
  p.o_mean = mean;
  p.o_invstd = invstd;
  p.o_scale = scale;
  p.o_shift = shift;
  const dim3 grid = ew_dims(p);
  CVHIP_LAUNCH_ACT_ACC(ew_kernel, 0, act, grid, (hipStream_t)stream, p)
  return check_launch("ew_kernel<0,acc>");
}

int cvhip_bn_finalize_acc(const double* acc, int32_t acc_ld, int32_t C, int64_t count, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, float momentum, float eps, float* mean, float* invstd, float* scale,
                          float* shift, void* stream) {
  if (!acc || !mean || !invstd || !scale || !shift || C <= 0 || count <= 0 || acc_ld < C) return CVHIP_ERR_INVALID;
  hipLaunchKernelGGL(bn_finalize_acc_kernel, dim3(cdiv(C, 256)), dim3(256), 0, (hipStream_t)stream, acc, acc_ld, C, (double)count, gamma, beta,
                     running_mean, running_var, momentum, eps, mean, invstd, scale, shift);
  return check_launch("bn_finalize_acc_kernel");
}

int cvhip_bn_act_fwd_acc_lazyres(const void* y, int32_t ld_y, void* z, int32_t ld_z, int64_t M, int32_t C, const double* acc, int32_t acc_ld,
                                 int64_t count, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                 float momentum, float eps, float* mean, float* invstd, float* scale, float* shift, int32_t act,
                                 float act_param, const void* residual_raw, int32_t ld_res, const float* res_scale, const float* res_shift,
                                 void* stream) {
  if (!y || !z || !acc || !mean || !invstd || !scale || !shift || M <= 0 || C <= 0 || count <= 0 || acc_ld < C) return CVHIP_ERR_INVALID;
  if (!residual_raw || !res_scale || !res_shift) return CVHIP_ERR_INVALID;
  if (C > kEwAccMaxC) return CVHIP_ERR_UNSUPPORTED;
  EwParams p{};
  p.a = (const h16_t*)y;
  p.ld_a = ld_y;
  p.out = (h16_t*)z;
  p.ld_out = ld_z;
  p.res = (const h16_t*)residual_raw;
  p.ld_res = ld_res;
  p.res_scale = res_scale;
  p.res_shift = res_shift;
  p.M = M;
  p.C = C;
  p.act = act;
  p.ap = act_param;
  p.acc = acc;
  p.acc_ld = acc_ld;
  p.count = (double)count;
  p.gamma = gamma;
  p.beta = beta;
  p.rmean = running_mean;
  p.rvar = running_var;
  p.momentum = momentum;
  p.eps = eps;
  p.o_mean = mean;
  p.o_invstd = invstd;
  p.o_scale = scale;
  p.o_shift = shift;
  const dim3 grid = ew_dims(p);
  switch (act) {
    case CVHIP_ACT_RELU: CVHIP_LAUNCH_A32(ew_kernel, grid, (hipStream_t)stream, p, 0, CVHIP_ACT_RELU, true, true); break;
    case CVHIP_ACT_SILU: CVHIP_LAUNCH_A32(ew_kernel, grid, (hipStream_t)stream, p, 0, CVHIP_ACT_SILU, true, true); break;
    case CVHIP_ACT_LEAKY: CVHIP_LAUNCH_A32(ew_kernel, grid, (hipStream_t)stream, p, 0, CVHIP_ACT_LEAKY, true, true); break;
    default: return CVHIP_ERR_UNSUPPORTED;
  }
  return check_launch("ew_kernel<0,acc,lazyres>");
}

int cvhip_bn_act_bwd_apply_acc(const void* dz, int32_t ld_dz, const void* y, int32_t ld_y, void* dy, int32_t ld_dy, int64_t M, int32_t C,
                               const float* scale, const float* shift, const float* mean, const float* invstd, const double* acc,
                               int32_t acc_ld, float* dgamma, float* dbeta, int32_t accumulate, int32_t act, float act_param, void* stream) {
  if (!dz || !y || !dy || !scale || !shift || !mean || !invstd || !acc || M <= 0 || C <= 0 || acc_ld < C) return CVHIP_ERR_INVALID;
  if (C > kEwAccMaxC) return CVHIP_ERR_UNSUPPORTED;
  EwParams p{};
  p.a = (const h16_t*)dz;
  p.ld_a = ld_dz;
  p.y = (const h16_t*)y;
  p.ld_y = ld_y;
  p.out = (h16_t*)dy;
  p.ld_out = ld_dy;
  p.M = M;
  p.C = C;
  p.scale = scale;
  p.shift = shift;
  p.mean = mean;
  p.invstd = invstd;
  p.act = act;
  p.ap = act_param;
  p.inv_count = 1.f / (float)M;
  p.acc = acc;
  p.acc_ld = acc_ld;
  p.o_dgamma = dgamma;
  p.o_dbeta = dbeta;
  p.accumulate = accumulate;
  const dim3 grid = ew_dims(p);
  CVHIP_LAUNCH_ACT_ACC(ew_kernel, 1, act, grid, (hipStream_t)stream, p)
  return check_launch("ew_kernel<1,acc>");
}

}  // extern "C"
