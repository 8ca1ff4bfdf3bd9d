// gnca_tangent.hip — forward-mode tangent (Jacobian-vector product) of the NCA step and of a whole
// scheduled rollout: gnca_step_tangent / gnca_rollout_tangent (include/gnca.h).
//
// One step x -> x' carries v -> v' with the conventions of the backward (the alive, sender and fire
// masks are constants, the perception bank is frozen, torus offset weights are the constant 1/k):
//
//   primal   the forward's own step (gnca_step_masked_phases, all phases): x', and in its workspace the
//            dense update field dxb and the GroupNorm partials
//   T0  gnca_t_prep      the pre-update alive / sender mask bytes of x, and (mu, rstd) per sample
//   TA  gnca_t_mlp       u' = fire * A_pre * (W2 ([hpre > 0] * W1 perceive(v)) + message tangent), dense,
//                        and per 32-cell tile the fp64 partials of sum u' and sum xhat * u'
//   TB  gnca_t_finalize  v' = v + gain * (1 - t^2) * GroupNorm'(u'), alpha gated by the post-update mask
//   TN  gnca_t_sumsq / gnca_t_lognorm / gnca_t_scale   at a tapped step: the log norm, renormalisation
//   TQ  gnca_t_gram / gnca_t_factor / gnca_t_apply     the thin QR of a block of K tangents (gnca_tangent_qr), which
//                        gnca_rollout_tangent_block runs at a tapped step; that rollout runs
//                        the primal step and T0 once per step and TA, TB once per direction
//   The *_params entry points carry a direction of the WEIGHTS beside v: TA's PT instances
//   add dW1 y, db1, dW2 relu(hpre), dWm s_x and dbm cnt from a second image set in LDS, TB adds dgamma xhat + dbeta.
//
// TA is persistent.  A wave owns 32 consecutive cells of one sample: the cells are the columns of
// v_mfma_f32_32x32x2_f32 tiles, so each of the 64 lanes holds one cell (lane & 31) and one of the two
// k values of a k-step (lane >> 5).  The weights sit in LDS in the order the A operand reads them;
// x and v are read straight from global memory (9 stencil taps per channel serve the identity and
// both Sobel features, for x and v alike), so there is no staged tile, no tile planner and no shape
// class without a plan.  The hidden layer's accumulator is the second product's B operand as it
// stands: a lane holds hidden rows (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) of each 32-row block, and the
// W2 image is read in that k order.
#include <algorithm>
#include <initializer_list>
#include <mutex>
#include <unordered_map>

#include "gnca_device.h"

namespace gnca {
namespace {

typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int kTile = 32;          // cells per wave tile (the MFMA's N)
constexpr int NW_ = kThreads / 64;  // waves per workgroup
constexpr uint32_t kTMsg = 1u << 8;   // the message term is on this step
constexpr uint32_t kTGN = 1u << 9;    // GroupNorm

__host__ __device__ inline int even2(int v) { return (v + 1) & ~1; }

// Masked loads.  A `keep ? load : 0` select (or its integer-mask form) lets the compiler branch around
// every load and wait out one memory latency per element.  The loads here are unconditional and the value
// is multiplied by a 0 / 1 float, which the compiler may not fold into a select, so a batch's loads are all
// in flight together.  Every masked-out load is redirected to an address whose value reaches the same
// output cell anyway: an off-image tap and a dead sender read the receiving cell itself, a padded channel
// reads a real channel of the same cell (C - 1 for the taps, 0 in the gather).  So a non-finite value under a
// zero mask (NaN where a select would give 0) can only be the cell's own, which makes its result NaN in any
// case; a NaN in a dead sender's cell does not reach the cells that would have heard from it.
// hidden row of accumulator register r of a 32x32 MFMA tile on lane half h
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

struct TLds {   // float offsets of the weight images in TA's dynamic LDS
  int HP, CPe, w1, b1, w2, wm, bm, wp, total;
};

__host__ __device__ inline TLds t_lds(int C, int hidden, int slice) {
  TLds L;
  L.CPe = even2(C);
  L.HP = (hidden + slice - 1) / slice * slice;
  L.w1 = 0;
  L.b1 = L.w1 + 3 * L.CPe * L.HP;
  L.w2 = L.b1 + L.HP;
  L.wm = L.w2 + L.HP * 32;
  L.bm = L.wm + L.CPe * 32;
  L.wp = L.bm + 32;
  L.total = L.wp + r4(27 * L.CPe);
  return L;
}

// ------------------------------------------------------------------------------------------
// T0: mask bytes of x (bit 0: pre-update alive, bit 1: sender alive) and the primal's (mu, rstd)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gnca_t_prep(const float* x, const double* stats, const uint8_t* active,
                                                       uint8_t* masks, float* coef, int C, int H, int W, int tps,
                                                       float thr, float gthr, float eps, int use_gn) {
  const int b = blockIdx.y;
  if (active && !active[b]) return;
  const size_t HW = (size_t)H * W;
  const float* a = x + ((size_t)b * C + 3) * HW;
  for (int cell = blockIdx.x * kThreads + threadIdx.x; cell < (int)HW; cell += gridDim.x * kThreads) {
    const int i = cell / W, j = cell - i * W;
    float mx = -INFINITY;
    for (int ii = max(0, i - 1); ii <= min(H - 1, i + 1); ++ii)
      for (int jj = max(0, j - 1); jj <= min(W - 1, j + 1); ++jj) mx = fmaxf(mx, a[(size_t)ii * W + jj]);
    masks[(size_t)b * HW + cell] = (uint8_t)((mx > thr ? 1 : 0) | (mx > gthr ? 2 : 0));
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    float mu = 0.f, rs = 1.f;
    if (use_gn) {
      double t1, t2;   // wave_sum2, as the forward K2: the same mean / rstd
      wave_sum2(stats + (size_t)b * tps * 2, tps, &t1, &t2);
      const double n = (double)C * (double)HW;
      const double m = t1 / n;
      double var = t2 / n - m * m;
      if (var < 0.0) var = 0.0;
      mu = (float)m;
      rs = (float)(1.0 / sqrt(var + (double)eps));
    }
    if (threadIdx.x == 0) {
      coef[2 * b] = mu;
      coef[2 * b + 1] = rs;
    }
  }
}

// ------------------------------------------------------------------------------------------
// TA: the tangent MLP kernel
// ------------------------------------------------------------------------------------------
struct TAArgs {
  const float* x;
  const float* v;
  const float* dx;        // the primal's dense update field (after fire and the pre mask)
  const uint8_t* masks;
  const float* coef;      // [B][2]: mu, rstd
  const void* fire;
  const uint8_t* active;
  const float *perc, *w1, *b1, *w2, *wm, *bm;
  float* ud;              // [B,C,H,W]: u', zeros at dead and unfired cells
  double* part;           // [B][ntile][2]: sum u', sum xhat u' of the tile
  int B, C, H, W, hidden, k, ntile, total, fire_mode;
  uint32_t flags;
  float fire_rate, message_gain, invk;
  uint64_t seed;
  int64_t rng_step, sample_base;
  int8_t off[2 * GNCA_MAX_OFFSETS];
  // the parameter direction (PT instances only; NULL = a zero direction for that tensor)
  const float *dw1, *db1, *dw2, *dwm, *dbm;
  int npass;              // hidden passes of a PT launch: 2 where both image sets of all hidden rows do not fit
};

constexpr int kPassRows = 128;   // hidden rows of one pass of a pass-staged PT launch (one NB = 4 slice)

// PT: beside v, a direction (dW1, db1, dW2, dWm, dbm) of the weights.  Its images sit
// behind the first set in the same order, and every term is one more MFMA into an accumulator that exists:
// dW1 y into accv, dW2 relu(hpre) into accu, dWm s_x into accd.  With npass == 2 the W1 / b1 / W2 images of
// both sets hold 128 hidden rows at a time: the pass loop is outside the tile loop, a wave visits the same
// tiles on the same lanes in both passes and parks accu in its own cells of ud between them.
template <int NB, bool PT>   // 32-row hidden blocks per slice
__global__ __launch_bounds__(kThreads) void gnca_t_mlp(const TAArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C, H = a.H, W = a.W, Hd = a.hidden;
  const int npass = PT ? a.npass : 1;
  const TLds L = t_lds(C, (PT && npass > 1) ? kPassRows : Hd, 32 * NB);
  const int HP = L.HP, CPe = L.CPe;
  float* w1s = smem + L.w1;
  float* b1s = smem + L.b1;
  float* w2s = smem + L.w2;
  float* wms = smem + L.wm;
  float* bms = smem + L.bm;
  float* wps = smem + L.wp;
  float* dset = smem + L.total;   // (PT) the second image set, at the first set's offsets
  const bool msg = (a.flags & kTMsg) != 0, gn = (a.flags & kTGN) != 0;
  // PT: the hidden passes, a backward jump at the end of the kernel (PT = false has no such loop around its tiles)
  int pass = 0;
next_pass:
  const int h0 = PT ? pass * HP : 0;   // the first hidden row of this pass's images
  const bool last = !PT || pass == npass - 1;
  if constexpr (PT) {
    if (pass > 0) __syncthreads();   // every wave is done with the previous pass's images
  }
  // weight images
  lds_fill<kThreads, 8>(w1s, 3 * CPe * HP, tid, [&](int idx) {
    const int kk = idx / HP, hid = h0 + idx - kk * HP, f = kk / CPe, c = kk - f * CPe;
    return (c < C && hid < Hd) ? a.w1[(size_t)hid * 3 * C + f * C + c] : 0.f;
  });
  lds_fill<kThreads, 4>(b1s, HP, tid, [&](int idx) { return h0 + idx < Hd ? a.b1[h0 + idx] : 0.f; });
  lds_fill<kThreads, 8>(w2s, HP * 32, tid, [&](int idx) {
    const int hid = h0 + (idx >> 5), co = idx & 31;
    return (co < C && hid < Hd) ? a.w2[(size_t)co * Hd + hid] : 0.f;
  });
  if (!PT || pass == 0) {
    lds_fill<kThreads, 4>(wms, CPe * 32, tid, [&](int idx) {
      const int ci = idx >> 5, co = idx & 31;
      return (msg && ci < C && co < C) ? a.wm[co * C + ci] : 0.f;
    });
    lds_fill<kThreads, 1>(bms, 32, tid, [&](int idx) { return (msg && idx < C) ? a.bm[idx] : 0.f; });
    lds_fill<kThreads, 4>(wps, 27 * CPe, tid, [&](int idx) { return idx < 27 * C ? a.perc[idx] : 0.f; });
  }
  if constexpr (PT) {
    lds_fill<kThreads, 8>(dset + L.w1, 3 * CPe * HP, tid, [&](int idx) {
      const int kk = idx / HP, hid = h0 + idx - kk * HP, f = kk / CPe, c = kk - f * CPe;
      return (a.dw1 && c < C && hid < Hd) ? a.dw1[(size_t)hid * 3 * C + f * C + c] : 0.f;
    });
    lds_fill<kThreads, 4>(dset + L.b1, HP, tid,
                          [&](int idx) { return (a.db1 && h0 + idx < Hd) ? a.db1[h0 + idx] : 0.f; });
    lds_fill<kThreads, 8>(dset + L.w2, HP * 32, tid, [&](int idx) {
      const int hid = h0 + (idx >> 5), co = idx & 31;
      return (a.dw2 && co < C && hid < Hd) ? a.dw2[(size_t)co * Hd + hid] : 0.f;
    });
    if (pass == 0) {
      lds_fill<kThreads, 4>(dset + L.wm, CPe * 32, tid, [&](int idx) {
        const int ci = idx >> 5, co = idx & 31;
        return (msg && a.dwm && ci < C && co < C) ? a.dwm[co * C + ci] : 0.f;
      });
      lds_fill<kThreads, 1>(dset + L.bm, 32, tid,
                            [&](int idx) { return (msg && a.dbm && idx < C) ? a.dbm[idx] : 0.f; });
    }
  }
  __syncthreads();

  const int col = lane & 31, h = lane >> 5;
  const int HW = H * W;
  const size_t sHW = (size_t)HW;
  for (int wt = blockIdx.x * NW_ + wave; wt < a.total; wt += gridDim.x * NW_) {
    const int b = wt / a.ntile, tile = wt - b * a.ntile;
    if (a.active && !a.active[b]) continue;
    const int cell = tile * kTile + col;
    const bool valid = cell < HW;
    const int i = valid ? cell / W : 0, j = valid ? cell - i * W : 0;
    const uint8_t* mb = a.masks + (size_t)b * sHW;
    const bool pre = valid && (mb[cell] & 1);
    const bool live = pre && fire_at(a.fire_mode, a.fire, a.fire_rate, a.seed, a.rng_step, a.sample_base, b, sHW,
                                     (size_t)cell);
    float* udb = a.ud + (size_t)b * C * sHW;
    double* outp = a.part + ((size_t)b * a.ntile + tile) * 2;
    if (__ballot(live) == 0ull) {   // nothing fires in this tile: u' = 0 (wave-uniform branch)
      if constexpr (PT) {
        if (!last) continue;   // (the last pass stores the zeros)
      }
      if (valid)
        for (int c = h; c < C; c += 2) udb[(size_t)c * sHW + cell] = 0.f;
      if (lane == 0) {
        outp[0] = 0.0;
        outp[1] = 0.0;
      }
      continue;
    }
    const float* xb = a.x + (size_t)b * C * sHW;
    const float* vb = a.v + (size_t)b * C * sHW;
    // the 9 stencil taps of this lane's cell (zero padding: perception.py:16)
    int nidx[9];
    bool nok[9];
    float nmask[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int ii = i + t / 3 - 1, jj = j + t % 3 - 1;
      nok[t] = valid && ii >= 0 && ii < H && jj >= 0 && jj < W;
      nidx[t] = nok[t] ? ii * W + jj : (valid ? cell : 0);
      nmask[t] = nok[t] ? 1.f : 0.f;
    }
    f16v accu;
#pragma unroll
    for (int r = 0; r < 16; ++r) accu[r] = 0.f;
    if constexpr (PT) {
      if (pass > 0) {   // the earlier passes' sum, parked by this lane in its own cells
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = acc_row(r, h);
          const float p = udb[(size_t)min(c, C - 1) * sHW + (valid ? cell : 0)];
          accu[r] = (c < C && valid) ? p : 0.f;   // (a lane without a cell or channel parked nothing)
        }
      }
    }
    for (int hb = 0; hb < HP; hb += 32 * NB) {
      f16v accy[NB], accv[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          accy[nb][r] = 0.f;
          accv[nb][r] = 0.f;
        }
      // hpre and W1 perceive(v): both B columns share one pass over the W1 image
      const int nsp = CPe / 2;
      auto load_taps = [&](int sp, float (&xo)[9], float (&vo)[9]) {   // raw: masked where they are used
        const int c = min(2 * sp + h, C - 1);
        const float* xc = xb + (size_t)c * sHW;
        const float* vc = vb + (size_t)c * sHW;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          xo[t] = xc[nidx[t]];
          vo[t] = vc[nidx[t]];
        }
      };
      auto products = [&](int sp, const float (&xi)[9], const float (&vi)[9]) {
        const int c = 2 * sp + h;
        const float cm = c < C ? 1.f : 0.f;
        float xm[9], vm[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          xm[t] = xi[t] * (nmask[t] * cm);
          vm[t] = vi[t] * (nmask[t] * cm);
        }
        const float* wp = wps + c * 27;   // (c < CPe: zeros past C)
#pragma unroll
        for (int f = 0; f < 3; ++f) {
          float y = 0.f, yd = 0.f;
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            const float wv = wp[f * 9 + t];
            y = fmaf(wv, xm[t], y);
            yd = fmaf(wv, vm[t], yd);
          }
          const float* wrow = w1s + (size_t)(f * CPe + c) * HP + hb + col;
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
            const float wa = wrow[32 * nb];
            accy[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa, y, accy[nb], 0, 0, 0);
            accv[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa, yd, accv[nb], 0, 0, 0);
            if constexpr (PT)   // dW1 y: the same y, another A fragment
              accv[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wrow[L.total + 32 * nb], y, accv[nb], 0, 0, 0);
          }
        }
      };
      // two tap sets: the next channel pair's 18 loads are issued before this pair's products
      float xa[9], va[9], xq[9], vq[9];
      load_taps(0, xa, va);
      for (int sp = 0; sp < nsp; sp += 2) {
        load_taps(min(sp + 1, nsp - 1), xq, vq);
        products(sp, xa, va);
        if (sp + 1 < nsp) {
          load_taps(min(sp + 2, nsp - 1), xa, va);
          products(sp + 1, xq, vq);
        }
      }
      // h' = [hpre > 0] * (W1 y'), then u' += W2 h' with the accumulator as the B operand
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int hid = hb + 32 * nb + acc_row(r, h);
          if constexpr (PT) {   // h' gains db1, and u' gains dW2 relu(hpre)
            const float hpre = accy[nb][r] + b1s[hid];
            const float hd = hpre > 0.f ? accv[nb][r] + dset[L.b1 + hid] : 0.f;
            accu = __builtin_amdgcn_mfma_f32_32x32x2f32(w2s[hid * 32 + col], hd, accu, 0, 0, 0);
            accu = __builtin_amdgcn_mfma_f32_32x32x2f32(dset[L.w2 + hid * 32 + col], fmaxf(hpre, 0.f), accu, 0, 0, 0);
          } else {
            const float hd = (accy[nb][r] + b1s[hid]) > 0.f ? accv[nb][r] : 0.f;
            accu = __builtin_amdgcn_mfma_f32_32x32x2f32(w2s[hid * 32 + col], hd, accu, 0, 0, 0);
          }
        }
    }
    if constexpr (PT) {
      if (!last) {   // park the partial sum; the message, the masks, the store and the partials are the last pass's
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = acc_row(r, h);
          if (c < C && valid) udb[(size_t)c * sHW + cell] = accu[r];
        }
        continue;
      }
    }
    // the message and its tangent: Wm (1/k sum_o shift_o(A_send z)) for z = x and z = v
    f16v accm, accd;
    float cnt = 0.f;
    if (msg) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        accm[r] = 0.f;
        accd[r] = 0.f;
      }
      const bool a2a = (a.flags & GNCA_ALIVE_TO_ALIVE) != 0;
      // four channel pairs per pass over the offsets, instead of one load latency per (channel pair, offset)
      for (int sp0 = 0; sp0 < CPe / 2; sp0 += 4) {
        float gx[4], gv[4];
        const float* xc[4];
        const float* vc[4];
        float cokf[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = 2 * (sp0 + u) + h;
          cokf[u] = (c < C && valid) ? 1.f : 0.f;
          xc[u] = xb + (size_t)(c < C ? c : 0) * sHW;
          vc[u] = vb + (size_t)(c < C ? c : 0) * sHW;
          gx[u] = 0.f;
          gv[u] = 0.f;
        }
        float ns = 0.f;
        // eight offsets at a time: their 8 mask bytes in one memory latency, then their 64 loads in another
        for (int o0 = 0; o0 < a.k; o0 += 8) {
          int q[8];
          uint8_t mq[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int o = min(o0 + e, a.k - 1);
            q[e] = wrapi(i - (int)a.off[2 * o], H) * W + wrapi(j - (int)a.off[2 * o + 1], W);
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) mq[e] = mb[q[e]];
          float xl[8][4], vl[8][4], sm[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const bool s = (o0 + e < a.k) & (!a2a | ((mq[e] & 2) != 0));
            sm[e] = s ? 1.f : 0.f;
            ns += (valid && s) ? 1.f : 0.f;
            q[e] = s ? q[e] : (valid ? cell : 0);   // a dead sender is not read: the cell itself, under a zero mask
          }
#pragma unroll
          for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              xl[e][u] = xc[u][q[e]];
              vl[e][u] = vc[u][q[e]];
            }
#pragma unroll
          for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              gx[u] = fmaf(xl[e][u], sm[e] * cokf[u], gx[u]);
              gv[u] = fmaf(vl[e][u], sm[e] * cokf[u], gv[u]);
            }
        }
        cnt = ns * a.invk;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = 2 * (sp0 + u) + h;   // (past CPe: a zero row of the padded Wm image is never read)
          const float wa = c < CPe ? wms[c * 32 + col] : 0.f;
          accm = __builtin_amdgcn_mfma_f32_32x32x2f32(wa, gx[u] * a.invk, accm, 0, 0, 0);
          accd = __builtin_amdgcn_mfma_f32_32x32x2f32(wa, gv[u] * a.invk, accd, 0, 0, 0);
          if constexpr (PT) {   // dWm s_x
            const float dwa = c < CPe ? dset[L.wm + c * 32 + col] : 0.f;
            accd = __builtin_amdgcn_mfma_f32_32x32x2f32(dwa, gx[u] * a.invk, accd, 0, 0, 0);
          }
        }
      }
    }
    // epilogue: the message tangent, the fire and pre masks, the dense store and the tile's partials
    float mu = 0.f, rs = 1.f;
    if (gn) {
      mu = a.coef[2 * b];
      rs = a.coef[2 * b + 1];
    }
    const float* dxb = a.dx + (size_t)b * C * sHW;
    const bool honly = (a.flags & GNCA_HIDDEN_ONLY) != 0;
    double su = 0.0, sux = 0.0;
    float dxv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {   // the 16 loads of the primal field together (clamped addresses)
      const int c = min(acc_row(r, h), C - 1);
      dxv[r] = gn ? dxb[(size_t)c * sHW + (valid ? cell : 0)] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = acc_row(r, h);
      const bool ok = c < C && valid;
      float u = accu[r];
      if (msg) {
        if constexpr (PT) {
          // the PT = false instance's roundings, spelled out (its compiler-chosen contractions: an FMA for m and
          // for 1 - tm^2, the gain's product rounded, and the sum an FMA except on the four registers whose
          // channel can be below 4, where the hidden-only select sits between product and sum), so that a zero
          // direction gives its bits whatever the vectoriser makes of this instance; dbm cnt joins accd in one
          // FMA, exact for dbm = 0
#pragma clang fp contract(off)
          const float tm = tanhf(fmaf(bms[min(c, 31)], cnt, accm[r]));
          const float om = fmaf(-tm, tm, 1.f);
          const float md = fmaf(dset[L.bm + min(c, 31)], cnt, accd[r]);
          const float gm = a.message_gain * om;
          if (r >= 4) {   // (c >= 8: never zeroed)
            u = fmaf(md, gm, u);
          } else {
            const float mt = md * gm;
            u += (honly && c < 4) ? 0.f : mt;
          }
        } else {
          const float tm = tanhf(accm[r] + bms[min(c, 31)] * cnt);
          u += (honly && c < 4) ? 0.f : a.message_gain * (1.f - tm * tm) * accd[r];
        }
      }
      u = (live && ok) ? u : 0.f;
      if (ok) udb[(size_t)c * sHW + cell] = u;
      const float xh = (dxv[r] - mu) * rs;
      su += (double)u;
      sux += (double)u * (double)xh;   // (u is 0 where the lane holds no cell or channel)
    }
    if (gn) {
      for (int off = 32; off > 0; off >>= 1) {
        su += __shfl_xor(su, off);
        sux += __shfl_xor(sux, off);
      }
      if (lane == 0) {
        outp[0] = su;
        outp[1] = sux;
      }
    }
  }
  if constexpr (PT) {
    if (++pass < npass) goto next_pass;
  }
}

// ------------------------------------------------------------------------------------------
// TB: GroupNorm tangent, tanh', residual and the alpha post gate (from x')
// ------------------------------------------------------------------------------------------
struct TBArgs {
  const float *x, *x_out, *v, *dx, *ud, *coef, *gamma, *beta;
  const double* part;
  const uint8_t* active;
  float* v_out;
  int B, C, H, W, ntile;
  float gain, thr;
  int use_gn;
  const float *dgamma, *dbeta;   // the direction of norm.weight / norm.bias (NULL = none)
};

__global__ __launch_bounds__(kThreads) void gnca_t_finalize(const TBArgs a) {
  __shared__ float sh[2];
  const int b = blockIdx.y, C = a.C, H = a.H, W = a.W;
  const int HW = H * W;
  const size_t sHW = (size_t)HW;
  const int cell = blockIdx.x * kThreads + threadIdx.x;
  const size_t base = (size_t)b * C * sHW;
  if (a.active && !a.active[b]) {   // the step left this sample alone: v passes through
    if (cell < HW)
      for (int c = 0; c < C; ++c) a.v_out[base + (size_t)c * sHW + cell] = a.v[base + (size_t)c * sHW + cell];
    return;
  }
  const bool gn = a.use_gn != 0;
  if (gn) {
    if (threadIdx.x < 64) {
      double su, sux;   // the tiles' partials in wave_sum2's fixed order
      wave_sum2(a.part + (size_t)b * a.ntile * 2, a.ntile, &su, &sux);
      const double n = (double)C * (double)HW;
      if (threadIdx.x == 0) {
        sh[0] = (float)(su / n);
        sh[1] = (float)(sux / n);
      }
    }
    __syncthreads();
  }
  if (cell >= HW) return;
  const float mu = gn ? a.coef[2 * b] : 0.f, rs = gn ? a.coef[2 * b + 1] : 1.f;
  const float mu_u = gn ? sh[0] : 0.f, mu_ux = gn ? sh[1] : 0.f;
  // post-update alive mask.  thr >= 0: from the gated alpha of x', exactly: a cell is alive iff a
  // neighbour's updated alpha exceeds thr, and that neighbour is then alive itself, so its alpha passed
  // the gate; a gated alpha is +-0 and never exceeds thr.  thr < 0: a gated +-0 would exceed it, so the
  // neighbours' updated alpha before the gate is recomputed with the forward K2's expression (as the
  // backward's BA does: the same gate bits)
  const int i = cell / W, j = cell - i * W;
  float mx = -INFINITY;
  if (a.thr >= 0.f) {
    const float* ao = a.x_out + base + 3 * sHW;
    for (int ii = max(0, i - 1); ii <= min(H - 1, i + 1); ++ii)
      for (int jj = max(0, j - 1); jj <= min(W - 1, j + 1); ++jj) mx = fmaxf(mx, ao[(size_t)ii * W + jj]);
  } else {
    const float* ax = a.x + base + 3 * sHW;
    const float* ad = a.dx + base + 3 * sHW;
    const float g3 = gn ? a.gamma[3] : 1.f, b3 = gn ? a.beta[3] : 0.f;
    for (int ii = max(0, i - 1); ii <= min(H - 1, i + 1); ++ii)
      for (int jj = max(0, j - 1); jj <= min(W - 1, j + 1); ++jj) {
        const size_t q = (size_t)ii * W + jj;
        float d = ad[q];
        if (gn) d = (d - mu) * rs * g3 + b3;
        mx = fmaxf(mx, ax[q] + fast_tanh(d) * a.gain);
      }
  }
  const float post = mx > a.thr ? 1.f : 0.f;
  for (int c = 0; c < C; ++c) {
    const size_t p = base + (size_t)c * sHW + cell;
    const float d = a.dx[p], u = a.ud[p], vv = a.v[p];
    float xn = d, un = u;
    if (gn) {
      const float gc = a.gamma[c], xh = (d - mu) * rs;
      xn = xh * gc + a.beta[c];
      un = gc * rs * (u - mu_u - xh * mu_ux);
      // the direction of the affine part, at every cell (GroupNorm runs on the masked field)
      if (a.dgamma || a.dbeta) un += (a.dgamma ? a.dgamma[c] : 0.f) * xh + (a.dbeta ? a.dbeta[c] : 0.f);
    }
    const float t = tanhf(xn);
    float o = vv + a.gain * (1.f - t * t) * un;
    if (c == 3) o *= post;
    a.v_out[p] = o;
  }
}

// ------------------------------------------------------------------------------------------
// TN: the log norm of a tapped step, and the renormalisation
// ------------------------------------------------------------------------------------------
constexpr int kNormChunk = 16 * kThreads;   // elements of one sample per workgroup

__global__ __launch_bounds__(kThreads) void gnca_t_sumsq(const float* v, double* pn, size_t n, int nchunk) {
  __shared__ double red[kThreads / 64];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const float* vb = v + (size_t)b * n;
  double s = 0.0;
  for (int u = 0; u < 16; ++u) {
    const size_t e = (size_t)chunk * kNormChunk + (size_t)u * kThreads + threadIdx.x;
    const double f = e < n ? (double)vb[e] : 0.0;
    s += f * f;
  }
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) pn[(size_t)b * nchunk + chunk] = ((red[0] + red[1]) + (red[2] + red[3]));
}

// one wave per sample: S = sum v'^2, log_norm = 0.5 log S + the carried log of earlier renormalisations
// (log_norm[b * stride]: the block rollout records direction j of [B][K] with stride K)
__global__ __launch_bounds__(64) void gnca_t_lognorm(const double* pn, int nchunk, double* carry, float* scale,
                                                     double* log_norm, int renorm, int stride) {
  const int b = blockIdx.x, lane = threadIdx.x;
  double s = 0.0;
  for (int t = lane; t < nchunk; t += 64) s += pn[(size_t)b * nchunk + t];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  s = __shfl(s, 0);
  if (lane != 0) return;
  const double half_log = 0.5 * log(s);   // -inf for a zero tangent
  log_norm[(size_t)b * stride] = half_log + carry[b];
  float sc = 1.f;
  if (renorm && s > 0.0 && s < INFINITY) {
    sc = (float)(1.0 / sqrt(s));
    carry[b] += half_log;
  }
  scale[b] = sc;
}

__global__ __launch_bounds__(kThreads) void gnca_t_scale(float* v, const float* scale, size_t n) {
  const int b = blockIdx.y;
  const float sc = scale[b];
  if (sc == 1.f) return;
  float* vb = v + (size_t)b * n;
  for (int u = 0; u < 16; ++u) {
    const size_t e = (size_t)blockIdx.x * kNormChunk + (size_t)u * kThreads + threadIdx.x;
    if (e < n) vb[e] *= sc;
  }
}

__global__ __launch_bounds__(kThreads) void gnca_t_zero_f64(double* p, int n) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) p[i] = 0.0;
}

// zero n 16-byte vectors: a workspace block (a multiple of 256 bytes on a 256-byte boundary).  A kernel, not a
// memset node, as gnca_rollout_bwd_taps' rows.
__global__ __launch_bounds__(kThreads) void gnca_t_zero_v4(float4* p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads)
    p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ------------------------------------------------------------------------------------------
// TQ: the thin QR of a tangent block v [K][B][n] (gnca_tangent_qr)
//   TQ1 gnca_t_gram    per (sample, chunk) the fp64 Gram partials of all K (K + 1) / 2 pairs
//   TQ2 gnca_t_factor  one wave per sample: G, its Cholesky factor with the pivot rule, Rinv, the logs
//   TQ3 gnca_t_apply   Q = V Rinv, in place
// ------------------------------------------------------------------------------------------
typedef double d4v __attribute__((ext_vector_type(4)));

constexpr int kMaxDirs = GNCA_TANGENT_MAX_DIRS;
constexpr int kQrChunk = GNCA_TANGENT_QR_CHUNK;   // elements of one sample per Gram workgroup
constexpr int kQrWave = kQrChunk / NW_;           // ... per wave: kQrWave / 4 k-steps of v_mfma_f64_16x16x4_f64
constexpr int kApplyPer = 2;                      // elements per thread of TQ3
constexpr int kApplyChunk = kApplyPer * kThreads;
static_assert(kMaxDirs == 16 && kQrWave % 32 == 0, "the Gram tile is the 16x16 MFMA's");

// The directions are the 16 rows AND the 16 columns of the MFMA (zero rows past K), the elements its k
// dimension: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], which for V^T V is one and
// the same value, direction l & 15 at element 4 s + (l >> 4) of k-step s.  A lane's load is 4 bytes and a
// wave's covers 16 B of each direction; the 8 k-steps in flight together cover 128 B of each.
__global__ __launch_bounds__(kThreads) void gnca_t_gram(const float* v, double* part, size_t n, size_t dstride,
                                                        int K, int nchunk) {
  __shared__ double red[NW_][256];
  const int b = blockIdx.x / nchunk, chunk = blockIdx.x - b * nchunk;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = lane & 15, kq = lane >> 4;
  const bool dok = d < K;
  const float* vd = v + (size_t)min(d, K - 1) * dstride + (size_t)b * n;
  const size_t e0 = (size_t)chunk * kQrChunk + (size_t)wave * kQrWave;
  d4v acc = {0.0, 0.0, 0.0, 0.0};
  for (int s0 = 0; s0 < kQrWave / 4; s0 += 8) {
    if (e0 + 4 * (size_t)s0 >= n) break;   // (wave-uniform)
    float f[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const size_t e = e0 + 4 * (size_t)(s0 + u) + kq;
      f[u] = vd[e < n ? e : n - 1];        // (clamped: never past the sample; the value is dropped below)
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const size_t e = e0 + 4 * (size_t)(s0 + u) + kq;
      const double a = (dok && e < n) ? (double)f[u] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, acc, 0, 0, 0);
    }
  }
  // C/D of the f64 MFMA: register g of lane l is row (l >> 4) + 4 g, column l & 15
#pragma unroll
  for (int g = 0; g < 4; ++g) red[wave][g * 64 + lane] = acc[g];
  __syncthreads();
  const int g = tid >> 6, row = (lane >> 4) + 4 * g, col = lane & 15;
  if (row <= col && col < K) {
    const int npair = K * (K + 1) / 2;
    part[((size_t)b * nchunk + chunk) * npair + col * (col + 1) / 2 + row] =
        (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  }
}

// One wave per sample.  rinv [B][16][16] (row-major, zero outside the kept rows and columns): every entry is
// written.  r / log_out / carry may be null; log_out[b][j] = log R_jj (+ carry[b][j], which then takes the log).
__global__ __launch_bounds__(64) void gnca_t_factor(const double* part, int nchunk, int K, double* rinv, double* r,
                                                    double* log_out, double* carry) {
  __shared__ double G[kMaxDirs][kMaxDirs + 1], R[kMaxDirs][kMaxDirs + 1], X[kMaxDirs][kMaxDirs + 1];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int npair = K * (K + 1) / 2;
  for (int idx = lane; idx < kMaxDirs * kMaxDirs; idx += 64) {
    const int i = idx >> 4, j = idx & 15;
    R[i][j] = 0.0;
    X[i][j] = 0.0;
    if (i <= j && j < K) {
      const double* p = part + (size_t)b * nchunk * npair + j * (j + 1) / 2 + i;
      double s = 0.0;
      for (int c = 0; c < nchunk; ++c) s += p[(size_t)c * npair];   // the chunks in order
      G[i][j] = s;
      G[j][i] = s;
    }
  }
  __syncthreads();
  const int k = lane;
  double logd = 0.0;   // lane j: log R_jj
  bool kept = false;   // lane j: column j was not dropped
  for (int j = 0; j < K; ++j) {
    const bool mine = k >= j && k < K;
    double s = 0.0;
    if (mine)
      for (int i = 0; i < j; ++i) s += R[i][j] * R[i][k];
    const double val = mine ? G[j][k] - s : 0.0;
    const double dj = __shfl(val, j);
    const bool ok = dj > 0.0 && dj < INFINITY && dj > 0x1p-44 * G[j][j];
    const double rjj = ok ? sqrt(dj) : 0.0;
    if (k == j) {
      kept = ok;
      logd = ok ? log(rjj) : -INFINITY;
    }
    if (k < kMaxDirs) R[j][k] = (ok && mine) ? (k == j ? rjj : val / rjj) : 0.0;
    __syncthreads();
  }
  // Rinv, column m on lane m: back substitution over the kept rows; dropped rows and columns stay zero
  if (k < K && kept) {
    const int m = k;
    X[m][m] = 1.0 / R[m][m];
    for (int i = m - 1; i >= 0; --i) {
      if (R[i][i] == 0.0) continue;
      double s = 0.0;
      for (int l = i + 1; l <= m; ++l) s += (R[l][l] == 0.0) ? 0.0 : R[i][l] * X[l][m];
      X[i][m] = -s / R[i][i];
    }
  }
  __syncthreads();
  for (int idx = lane; idx < kMaxDirs * kMaxDirs; idx += 64) {
    const int i = idx >> 4, j = idx & 15;
    rinv[(size_t)b * kMaxDirs * kMaxDirs + idx] = X[i][j];
    if (r && i < K && j < K) r[((size_t)b * K + i) * K + j] = R[i][j];
  }
  if (k < K && log_out) {
    const size_t o = (size_t)b * K + k;
    if (carry) {
      log_out[o] = logd + carry[o];
      if (kept) carry[o] += logd;
    } else {
      log_out[o] = logd;
    }
  }
}

// KB: K rounded up to 4, 8 or 16 (the unrolled triangle).  A thread reads its element's K values, one per
// direction (a wave's loads of one direction are 256 contiguous bytes), and stores K.
template <int KB>
__global__ __launch_bounds__(kThreads) void gnca_t_apply(float* v, const double* rinv, size_t n, size_t dstride,
                                                         int K, int nchunk) {
  __shared__ double X[kMaxDirs * kMaxDirs];
  const int b = blockIdx.x / nchunk, chunk = blockIdx.x - b * nchunk;
  X[threadIdx.x] = rinv[(size_t)b * kMaxDirs * kMaxDirs + threadIdx.x];
  __syncthreads();
  float* vb = v + (size_t)b * n;
  float f[kApplyPer][KB];
#pragma unroll
  for (int u = 0; u < kApplyPer; ++u) {
    const size_t e = (size_t)chunk * kApplyChunk + (size_t)u * kThreads + threadIdx.x;
#pragma unroll
    for (int i = 0; i < KB; ++i) f[u][i] = vb[(size_t)min(i, K - 1) * dstride + (e < n ? e : n - 1)];
  }
#pragma unroll
  for (int u = 0; u < kApplyPer; ++u) {
    const size_t e = (size_t)chunk * kApplyChunk + (size_t)u * kThreads + threadIdx.x;
    double a[KB];
#pragma unroll
    for (int i = 0; i < KB; ++i) a[i] = (i < K && X[i * kMaxDirs + i] != 0.0) ? (double)f[u][i] : 0.0;   // a dropped row is skipped
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      double q = 0.0;
#pragma unroll
      for (int i = 0; i <= j; ++i) q = fma(a[i], X[i * kMaxDirs + j], q);
      if (j < K && e < n) vb[(size_t)j * dstride + e] = (float)q;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Host
// ------------------------------------------------------------------------------------------
// a runtime call's status as a return code; a failure is kept for gnca_last_hip_error
int t_hip(hipError_t e) {
  if (e == hipSuccess) return GNCA_OK;
  g_last_hip = (int)e;
  return GNCA_ERR_HIP;
}

int t_check() { return t_hip(hipGetLastError()); }

int t_device_cus() {
  static std::mutex mu;
  static std::unordered_map<int, int> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(dev);
  if (it != cache.end()) return it->second;
  int cus = 256;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
  cache[dev] = cus;
  return cus;
}

// The step's workspace: [forward step workspace | u' | mask bytes | coef | tile partials]
struct TanLayout {
  FwdLayout F;
  size_t off_fwd, off_ud, off_masks, off_coef, off_part, bytes;
  int ntile, NB;
  bool msg, gn;
};

bool tangent_unsupported(const gnca_step_desc* d) {
  return (d->flags & GNCA_GRAPH) && (d->flags & GNCA_ZERO_PAD_SHIFT) && d->num_offsets > 0;
}

// a well-formed shape outside the compiled support set (gnca_status_string names it)
bool outside_support(const gnca_step_desc* d) {
  if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->C < 4 || d->hidden <= 0) return false;
  return d->C > 32 || d->hidden > ((d->C >= 13 && d->C <= 16) ? 256 : 128);
}

bool tan_layout(const gnca_step_desc* desc, TanLayout* T) {
  if (!desc) return false;
  gnca_step_desc d = *desc;
  d.flags &= ~GNCA_ATTENTION;
  if (tangent_unsupported(&d)) return false;
  if (!fwd_layout(&d, &T->F)) return false;
  const size_t HW = (size_t)d.H * d.W, n = (size_t)d.B * d.C * HW;
  T->ntile = (int)((HW + kTile - 1) / kTile);
  if ((size_t)d.B * T->ntile > 0x7fffffffull) return false;
  T->NB = d.hidden <= 32 ? 1 : d.hidden <= 64 ? 2 : 4;
  T->msg = (d.flags & GNCA_GRAPH) && d.num_offsets > 0 && d.message_gain != 0.f;
  T->gn = (d.flags & GNCA_USE_GROUPNORM) != 0;
  size_t o = 0;
  T->off_fwd = o;   o += align256(T->F.ws_bytes);
  T->off_ud = o;    o += align256(n * sizeof(float));
  T->off_masks = o; o += align256((size_t)d.B * HW);
  T->off_coef = o;  o += align256((size_t)d.B * 2 * sizeof(float));
  T->off_part = o;  o += align256((size_t)d.B * T->ntile * 2 * sizeof(double));
  T->bytes = o;
  return true;
}

// the largest step workspace of a schedule (the forward plan varies with the message and the offsets' reach)
bool tan_sched_bytes(const gnca_step_desc* d, const gnca_rollout_sched* s, size_t* out) {
  TanLayout T;
  if (!tan_layout(d, &T)) return false;
  size_t m = T.bytes;
  uint32_t seen[64];
  int ns = 0;
  for (int t = 0; t < s->steps; ++t) {
    gnca_step_desc sd;
    sched_step_desc(d, s, t, &sd);
    int ry = 0, rx = 0;
    for (int o = 0; o < sd.num_offsets; ++o) {
      ry = std::max(ry, std::abs((int)sd.offsets[2 * o]));
      rx = std::max(rx, std::abs((int)sd.offsets[2 * o + 1]));
    }
    const uint32_t key = (sd.message_gain != 0.f ? 1u << 16 : 0u) | ((uint32_t)ry << 8) | (uint32_t)rx;
    bool hit = false;
    for (int q = 0; q < ns; ++q) hit = hit || seen[q] == key;
    if (hit) continue;
    if (ns < 64) seen[ns++] = key;
    if (!tan_layout(&sd, &T)) return false;
    m = std::max(m, T.bytes);
  }
  *out = m;
  return true;
}

// LDS floats of a PT launch: the second image set (no second perception bank) behind the first
inline int t_lds_pt(const TLds& L) { return L.total + L.wp; }

// the passes of a PT launch: both image sets of every class up to 128 hidden rows fit the CU's 160 KiB (p31: 140.6
// KiB); the hidden > 128 classes (13 <= C <= 16, up to 167.9 KiB in one piece) take 128 rows at a time
inline int t_passes(int hidden) { return hidden <= kPassRows ? 1 : (hidden + kPassRows - 1) / kPassRows; }

template <int NB, bool PT>
int launch_ta(const TAArgs& a, int C, int hidden, hipStream_t st) {
  const TLds L = t_lds(C, (PT && a.npass > 1) ? kPassRows : hidden, 32 * NB);
  const size_t lds = (size_t)(PT ? t_lds_pt(L) : L.total) * sizeof(float);
  auto fn = gnca_t_mlp<NB, PT>;
  // the dynamic-LDS attribute and the resident workgroups per CU (registers and LDS decide), set and asked
  // once per (device, LDS size)
  static std::mutex mu;
  static std::unordered_map<uint64_t, int> cache;
  int per_cu = 0, dev = 0;
  (void)hipGetDevice(&dev);
  {
    std::lock_guard<std::mutex> lk(mu);
    const uint64_t key = ((uint64_t)(uint32_t)dev << 32) | (uint64_t)lds;
    auto it = cache.find(key);
    if (it != cache.end()) per_cu = it->second;
    else {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds);
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(fn), kThreads, lds) !=
              hipSuccess || per_cu < 1)
        per_cu = 1;
      cache[key] = per_cu = std::min(per_cu, 2);
    }
  }
  const long want = ((long)a.total + NW_ - 1) / NW_;
  const int grid = (int)std::max<long>(1, std::min<long>(want, (long)t_device_cus() * per_cu));
  hipLaunchKernelGGL(fn, dim3(grid), dim3(kThreads), lds, st, a);
  return t_check();
}

// One step and its tangent, in two parts that share the step workspace: the primal part (the forward's step and
// T0) once per step, the direction part (TA, TB) once per tangent carried through that step.
int step_tangent_primal(const gnca_step_desc* desc, const gnca_weights* w, const float* x, const void* fire,
                        const uint8_t* active, float* x_out, void* ws, size_t ws_bytes, hipStream_t st) {
  gnca_step_desc d = *desc;
  d.flags &= ~GNCA_ATTENTION;
  TanLayout T;
  if (!tan_layout(&d, &T)) return GNCA_ERR_INVALID;
  if (!ws || ws_bytes < T.bytes) return GNCA_ERR_WORKSPACE;
  char* wsb = reinterpret_cast<char*>(ws);
  int rc = gnca_step_masked_phases(&d, w, x, x_out, fire, active, wsb + T.off_fwd, T.F.ws_bytes, st, GNCA_PHASE_ALL);
  if (rc != GNCA_OK) return rc;
  const int B = d.B, C = d.C, H = d.H, W = d.W;
  const int HW = H * W;
  const double* stats = reinterpret_cast<const double*>(wsb + T.off_fwd + T.F.off_stats);
  uint8_t* masks = reinterpret_cast<uint8_t*>(wsb + T.off_masks);
  float* coef = reinterpret_cast<float*>(wsb + T.off_coef);
  const int ncb = (HW + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(gnca_t_prep, dim3((unsigned)std::min(ncb, 64), (unsigned)B), dim3(kThreads), 0, st, x, stats,
                     active, masks, coef, C, H, W, T.F.tps, d.alpha_thr, d.graph_alpha_thr, d.gn_eps, T.gn ? 1 : 0);
  return t_check();
}

// v -> v_out through the step whose primal part has just run in `ws` (x, x_out, fire, active as passed there)
// dw: the parameter direction carried beside v (gnca_step_tangent_params), or NULL: the state tangent alone
int step_tangent_dir(const gnca_step_desc* desc, const gnca_weights* w, const gnca_weights* dw, const float* x,
                     const void* fire, const uint8_t* active, const float* v, const float* x_out, float* v_out,
                     void* ws, hipStream_t st) {
  gnca_step_desc d = *desc;
  d.flags &= ~GNCA_ATTENTION;
  TanLayout T;
  if (!tan_layout(&d, &T)) return GNCA_ERR_INVALID;
  char* wsb = reinterpret_cast<char*>(ws);
  int rc;
  const int B = d.B, C = d.C, H = d.H, W = d.W;
  const int HW = H * W;
  const float* dx = reinterpret_cast<const float*>(wsb + T.off_fwd + T.F.off_dx);
  float* ud = reinterpret_cast<float*>(wsb + T.off_ud);
  uint8_t* masks = reinterpret_cast<uint8_t*>(wsb + T.off_masks);
  float* coef = reinterpret_cast<float*>(wsb + T.off_coef);
  double* part = reinterpret_cast<double*>(wsb + T.off_part);
  const int ncb = (HW + kThreads - 1) / kThreads;
  {
    TAArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.v = v; a.dx = dx; a.masks = masks; a.coef = coef; a.fire = fire; a.active = active;
    a.perc = w->perception; a.w1 = w->w1; a.b1 = w->b1; a.w2 = w->w2; a.wm = w->wm; a.bm = w->bm;
    a.ud = ud; a.part = part;
    a.B = B; a.C = C; a.H = H; a.W = W; a.hidden = d.hidden; a.k = T.msg ? d.num_offsets : 0;
    a.ntile = T.ntile; a.total = B * T.ntile; a.fire_mode = d.fire_mode;
    a.flags = (d.flags & (GNCA_ALIVE_TO_ALIVE | GNCA_HIDDEN_ONLY)) | (T.msg ? kTMsg : 0u) | (T.gn ? kTGN : 0u);
    a.fire_rate = d.fire_rate; a.message_gain = d.message_gain;
    a.invk = a.k > 0 ? (float)(1.0 / (double)a.k) : 0.f;
    a.seed = d.rng_seed; a.rng_step = d.rng_step; a.sample_base = d.sample_base;
    for (int o = 0; o < 2 * a.k; ++o) a.off[o] = d.offsets[o];
    if (dw) {
      a.dw1 = dw->w1; a.db1 = dw->b1; a.dw2 = dw->w2; a.dwm = dw->wm; a.dbm = dw->bm;
      a.npass = t_passes(d.hidden);
      rc = T.NB == 1 ? launch_ta<1, true>(a, C, d.hidden, st)
                     : T.NB == 2 ? launch_ta<2, true>(a, C, d.hidden, st) : launch_ta<4, true>(a, C, d.hidden, st);
    } else {
      rc = T.NB == 1 ? launch_ta<1, false>(a, C, d.hidden, st)
                     : T.NB == 2 ? launch_ta<2, false>(a, C, d.hidden, st) : launch_ta<4, false>(a, C, d.hidden, st);
    }
    if (rc != GNCA_OK) return rc;
  }
  {
    TBArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.x_out = x_out; a.v = v; a.dx = dx; a.ud = ud; a.coef = coef; a.gamma = w->gn_weight; a.beta = w->gn_bias;
    a.part = part; a.active = active; a.v_out = v_out;
    a.B = B; a.C = C; a.H = H; a.W = W; a.ntile = T.ntile;
    a.gain = d.update_gain; a.thr = d.alpha_thr; a.use_gn = T.gn ? 1 : 0;
    if (dw && T.gn) {
      a.dgamma = dw->gn_weight;
      a.dbeta = dw->gn_bias;
    }
    hipLaunchKernelGGL(gnca_t_finalize, dim3((unsigned)ncb, (unsigned)B), dim3(kThreads), 0, st, a);
    if ((rc = t_check()) != GNCA_OK) return rc;
  }
  return GNCA_OK;
}

// the body of gnca_step_tangent and of gnca_rollout_tangent's steps
int step_tangent_impl(const gnca_step_desc* desc, const gnca_weights* w, const gnca_weights* dw, const float* x,
                      const void* fire, const uint8_t* active, const float* v, float* x_out, float* v_out, void* ws,
                      size_t ws_bytes, hipStream_t st) {
  const int rc = step_tangent_primal(desc, w, x, fire, active, x_out, ws, ws_bytes, st);
  if (rc != GNCA_OK) return rc;
  return step_tangent_dir(desc, w, dw, x, fire, active, v, x_out, v_out, ws, st);
}

// the outputs (null: not asked for) differ from one another, from the inputs x and v, and from every tensor of
// the directions dw[0..K) (dw null: none)
bool outputs_distinct(std::initializer_list<const void*> outs, const void* x, const void* v, const gnca_weights* dw,
                      int K) {
  for (auto o = outs.begin(); o != outs.end(); ++o) {
    if (!*o) continue;
    if (*o == x || *o == v) return false;
    for (auto q = o + 1; q != outs.end(); ++q)
      if (*o == *q) return false;
    for (int j = 0; dw && j < K; ++j) {
      const float* t[] = {dw[j].w1, dw[j].b1, dw[j].w2, dw[j].gn_weight, dw[j].gn_bias, dw[j].wm, dw[j].bm};
      for (const float* p : t)
        if (p == *o) return false;
    }
  }
  return true;
}

bool records_ok(const gnca_rollout_sched* s, const gnca_tangent_args* a) {
  if (!a || a->num_records < 0) return false;
  if (a->flags & ~(uint32_t)GNCA_TANGENT_RENORM) return false;
  if (a->num_records == 0) return true;
  if (!a->record) return false;
  int prev = 0;
  for (int r = 0; r < a->num_records; ++r) {
    if (a->record[r] <= prev || a->record[r] > s->steps) return false;
    prev = a->record[r];
  }
  return true;
}

// a well-formed schedule whose flags suit the entry: the Gauss-Newton forward writes a states-only tape
// (RECOMPUTE, with or without CHECKPOINT), the other tangent rollouts have no tape at all
bool tan_sched_ok(const gnca_step_desc* d, const gnca_rollout_sched* s, bool tape) {
  if (!sched_ok(d, s)) return false;
  return tape ? (s->flags & GNCA_SCHED_RECOMPUTE) != 0
              : !(s->flags & (GNCA_SCHED_RECOMPUTE | GNCA_SCHED_CHECKPOINT));
}

// What every tangent rollout's workspace begins with:
// [masks [T][B] | step workspace | nstate x states | 2 x K tangents]; an entry's own blocks follow at `bytes`.
// nstate: the ping-pong primal states, 2, or 0 when every state goes to an un-checkpointed tape.
struct TanRollLayout {
  size_t masks, step_ws, state, block, bytes;
  int nstate;
};

bool tan_roll_layout(const gnca_step_desc* d, const gnca_rollout_sched* s, int K, int nstate, TanRollLayout* R) {
  if (K < 1 || K > kMaxDirs) return false;
  size_t sw;
  if (!tan_sched_bytes(d, s, &sw)) return false;
  const size_t n = (size_t)d->C * d->H * d->W;
  R->masks = align256((size_t)std::max(s->steps, 1) * d->B);
  R->step_ws = align256(sw);
  R->state = align256((size_t)d->B * n * sizeof(float));
  R->block = align256((size_t)K * d->B * n * sizeof(float));
  R->nstate = nstate;
  R->bytes = R->masks + R->step_ws + (size_t)nstate * R->state + 2 * R->block;
  return true;
}

// gnca_rollout_tangent: the prefix, then [norm partials | carry | scale]
struct RollTanLayout {
  TanRollLayout R;
  size_t off_pn, off_carry, off_scale, bytes;
  int nchunk;
};

bool roll_tan_layout(const gnca_step_desc* d, const gnca_rollout_sched* s, const gnca_tangent_args* a,
                     RollTanLayout* L) {
  if (!tan_sched_ok(d, s, false) || !records_ok(s, a) || !tan_roll_layout(d, s, 1, 2, &L->R)) return false;
  const size_t n = (size_t)d->C * d->H * d->W;
  L->nchunk = (int)((n + kNormChunk - 1) / kNormChunk);
  size_t o = L->R.bytes;
  L->off_pn = o;    o += align256((size_t)d->B * L->nchunk * sizeof(double));
  L->off_carry = o; o += align256((size_t)d->B * sizeof(double));
  L->off_scale = o; o += align256((size_t)d->B * sizeof(float));
  L->bytes = o;
  return true;
}

// gnca_tangent_qr's workspace: [Gram partials [B][nchunk][K (K + 1) / 2] | Rinv [B][16][16]]
struct QrLayout {
  size_t off_rinv, bytes;
  int nchunk, napply;
};

bool qr_layout(int K, int B, int64_t n, QrLayout* Q) {
  if (K < 1 || K > kMaxDirs || B < 1 || n < 1) return false;
  const int64_t nchunk = (n + kQrChunk - 1) / kQrChunk, napply = (n + kApplyChunk - 1) / kApplyChunk;
  if (napply * (int64_t)B > 0x7fffffffll) return false;   // (the grids are one-dimensional)
  Q->nchunk = (int)nchunk;
  Q->napply = (int)napply;
  // (room for 16 directions' pairs whatever K: the block rollout's workspace is then linear in K)
  Q->off_rinv = align256((size_t)B * (size_t)nchunk * (size_t)(kMaxDirs * (kMaxDirs + 1) / 2) * sizeof(double));
  Q->bytes = Q->off_rinv + align256((size_t)B * kMaxDirs * kMaxDirs * sizeof(double));
  return true;
}

// TQ1, TQ2, TQ3 on v [K] directions `dstride` elements apart; r / log_out / carry as gnca_t_factor takes them
int launch_qr(const QrLayout& Q, int K, int B, size_t n, size_t dstride, float* v, double* r, double* log_out,
              double* carry, char* qws, hipStream_t st) {
  double* part = reinterpret_cast<double*>(qws);
  double* rinv = reinterpret_cast<double*>(qws + Q.off_rinv);
  int rc;
  hipLaunchKernelGGL(gnca_t_gram, dim3((unsigned)((size_t)B * Q.nchunk)), dim3(kThreads), 0, st, (const float*)v, part,
                     n, dstride, K, Q.nchunk);
  if ((rc = t_check()) != GNCA_OK) return rc;
  hipLaunchKernelGGL(gnca_t_factor, dim3((unsigned)B), dim3(64), 0, st, (const double*)part, Q.nchunk, K, rinv, r,
                     log_out, carry);
  if ((rc = t_check()) != GNCA_OK) return rc;
  const dim3 g((unsigned)((size_t)B * Q.napply));
  if (K <= 4)
    hipLaunchKernelGGL(gnca_t_apply<4>, g, dim3(kThreads), 0, st, v, (const double*)rinv, n, dstride, K, Q.napply);
  else if (K <= 8)
    hipLaunchKernelGGL(gnca_t_apply<8>, g, dim3(kThreads), 0, st, v, (const double*)rinv, n, dstride, K, Q.napply);
  else
    hipLaunchKernelGGL(gnca_t_apply<16>, g, dim3(kThreads), 0, st, v, (const double*)rinv, n, dstride, K, Q.napply);
  return t_check();
}

bool block_records_ok(const gnca_rollout_sched* s, const gnca_tangent_block_args* a) {
  if (!a || a->num_dirs < 1 || a->num_dirs > kMaxDirs) return false;
  if (a->flags & ~(uint32_t)GNCA_TBLOCK_ORTHO) return false;
  gnca_tangent_args one;
  memset(&one, 0, sizeof(one));
  one.num_records = a->num_records;
  one.record = a->record;
  return records_ok(s, &one);
}

// gnca_rollout_tangent_block: the prefix, then [norm partials | scale | carry [B][16] | QR workspace]
struct BlockTanLayout {
  TanRollLayout R;
  size_t off_pn, off_scale, off_carry, off_qr, bytes;
  int nchunk;
  QrLayout Q;
};

bool block_tan_layout(const gnca_step_desc* d, const gnca_rollout_sched* s, const gnca_tangent_block_args* a,
                      BlockTanLayout* L) {
  if (!tan_sched_ok(d, s, false) || !block_records_ok(s, a) || !tan_roll_layout(d, s, a->num_dirs, 2, &L->R))
    return false;
  const size_t n = (size_t)d->C * d->H * d->W;
  if (!qr_layout(a->num_dirs, d->B, (int64_t)n, &L->Q)) return false;
  L->nchunk = (int)((n + kNormChunk - 1) / kNormChunk);
  size_t o = L->R.bytes;
  L->off_pn = o;    o += align256((size_t)d->B * L->nchunk * sizeof(double));
  L->off_scale = o; o += align256((size_t)d->B * sizeof(float));
  L->off_carry = o; o += align256((size_t)d->B * kMaxDirs * sizeof(double));
  L->off_qr = o;    o += L->Q.bytes;
  L->bytes = o;
  return true;
}

// gnca_rollout_objective_tangent: the prefix alone
bool obj_tan_layout(const gnca_step_desc* d, const gnca_rollout_sched* s, const gnca_rollout_taps* taps, int K,
                    TanRollLayout* R) {
  return tan_sched_ok(d, s, false) && taps_ok(d, s, taps) && tan_roll_layout(d, s, K, 2, R);
}

// gnca_rollout_gn_fwd: the prefix for one direction, and the tape.  The primal's states go to the tape; only a
// checkpointed schedule needs the two ping-pong states for the ones between two anchors.
struct GnFwdLayout {
  TanRollLayout R;
  TapeLayout T;
};

bool gn_fwd_layout(const gnca_step_desc* d, const gnca_rollout_sched* s, const gnca_rollout_taps* taps,
                   GnFwdLayout* L) {
  return tan_sched_ok(d, s, true) && taps_ok(d, s, taps) && tape_layout(d, s, &L->T) &&
         tan_roll_layout(d, s, 1, L->T.k > 0 ? 2 : 0, &L->R);
}

// The refusals every tangent rollout entry shares once its own arguments have passed, in the order they win.
// tape: as tan_sched_ok; laid_out: the entry's layout exists; fits: the caller's buffers hold it.
int tan_roll_check(const gnca_step_desc* d, const gnca_rollout_sched* s, bool tape, bool laid_out, bool fits) {
  if (!tan_sched_ok(d, s, tape)) return GNCA_ERR_INVALID;
  if (tangent_unsupported(d)) return GNCA_ERR_UNSUPPORTED;
  if (!laid_out) return outside_support(d) ? GNCA_ERR_UNSUPPORTED : GNCA_ERR_INVALID;
  if (!fits) return GNCA_ERR_WORKSPACE;
  if ((d->fire_mode == GNCA_FIRE_RAND_F32 || d->fire_mode == GNCA_FIRE_MASK_U8) && s->steps > 0 && !s->fire)
    return GNCA_ERR_INVALID;
  return GNCA_OK;
}

// One rollout of the step and K tangents of it.
struct TanRoll {
  int K;
  const gnca_weights* dw;      // [K] weight directions, or null: state tangents alone
  const float *x, *v;          // v null: a zero block, made on the device
  float *x_final, *v_final;    // v_final null: the last tangents stay in the workspace
  char* tape;                  // the states-only tape (slot 0 takes a copy of x), or null: ping-pong states only
  size_t slot;                 // ... its slot size
  int every;                   // ... its anchor interval, 0: every state has a slot
  double* carry;               // ncarry log-norm carries to zero before the first step, or null
  int ncarry;
};

// After step t has written (xn, vn [K]), `after(t, xn, vn)` records what the entry records there; its return
// code, unless GNCA_OK, ends the rollout.  Zero steps copy the inputs out.
template <class After>
int tangent_rollout(const gnca_step_desc* desc, const gnca_weights* w, const gnca_rollout_sched* sched,
                    const TanRollLayout& R, char* wsb, const TanRoll& a, hipStream_t st, After&& after) {
  const int T = sched->steps, B = desc->B, K = a.K;
  const size_t dstride = (size_t)B * desc->C * desc->H * desc->W, nbytes = dstride * sizeof(float);
  int rc;
  if (T == 0) {
    if ((rc = t_hip(hipMemcpyAsync(a.x_final, a.x, nbytes, hipMemcpyDeviceToDevice, st))) != GNCA_OK) return rc;
    return t_hip(hipMemcpyAsync(a.v_final, a.v, (size_t)K * nbytes, hipMemcpyDeviceToDevice, st));
  }
  uint8_t* masks = reinterpret_cast<uint8_t*>(wsb);
  char* step_ws = wsb + R.masks;
  float* xp[2] = {nullptr, nullptr}, *vp[2];
  for (int q = 0; q < 2; ++q) {
    if (R.nstate) xp[q] = reinterpret_cast<float*>(wsb + R.masks + R.step_ws + (size_t)q * R.state);
    vp[q] = reinterpret_cast<float*>(wsb + R.masks + R.step_ws + (size_t)R.nstate * R.state + (size_t)q * R.block);
  }
  if (sched->nsteps && (rc = launch_nsteps_masks(sched->nsteps, B, T, sched->full_steps, masks, st)) != GNCA_OK)
    return rc;
  const float* xc = a.x;
  if (a.tape) {   // the tape stands alone: slot 0 keeps its own copy of x, and step 0 reads it there
    if ((rc = t_hip(hipMemcpyAsync(a.tape, a.x, nbytes, hipMemcpyDeviceToDevice, st))) != GNCA_OK) return rc;
    xc = reinterpret_cast<const float*>(a.tape);
  }
  const float* vc = a.v;
  if (!vc) {   // the zero block: step 0 reads vp[1] and writes vp[0]
    const size_t nv = R.block / sizeof(float4);
    hipLaunchKernelGGL(gnca_t_zero_v4, dim3((unsigned)std::min<size_t>((nv + kThreads - 1) / kThreads, 4096)),
                       dim3(kThreads), 0, st, reinterpret_cast<float4*>(vp[1]), nv);
    if ((rc = t_check()) != GNCA_OK) return rc;
    vc = vp[1];
  }
  if (a.carry) {
    hipLaunchKernelGGL(gnca_t_zero_f64, dim3((unsigned)((a.ncarry + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       a.carry, a.ncarry);
    if ((rc = t_check()) != GNCA_OK) return rc;
  }
  for (int t = 0; t < T; ++t) {
    gnca_step_desc sd;
    sched_step_desc(desc, sched, t, &sd);
    float* xn;
    if (t == T - 1) xn = a.x_final;
    else if (!a.tape) xn = xp[t & 1];
    else if (a.every == 0) xn = reinterpret_cast<float*>(a.tape + (size_t)(t + 1) * a.slot);
    else xn = (t + 1) % a.every == 0 ? reinterpret_cast<float*>(a.tape + (size_t)((t + 1) / a.every) * a.slot)
                                     : xp[t & 1];
    float* vn = (t == T - 1 && a.v_final) ? a.v_final : vp[t & 1];
    const void* fire = sched_step_fire(desc, sched, t);
    const uint8_t* active = sched_step_active(desc, sched, t, masks);
    if ((rc = step_tangent_primal(&sd, w, xc, fire, active, xn, step_ws, R.step_ws, st)) != GNCA_OK) return rc;
    for (int j = 0; j < K; ++j)
      if ((rc = step_tangent_dir(&sd, w, a.dw ? a.dw + j : nullptr, xc, fire, active, vc + (size_t)j * dstride, xn,
                                 vn + (size_t)j * dstride, step_ws, st)) != GNCA_OK)
        return rc;
    xc = xn;
    vc = vn;
    if ((rc = after(t, xn, vn)) != GNCA_OK) return rc;
  }
  return GNCA_OK;
}

}  // namespace
}  // namespace gnca

using namespace gnca;

extern "C" {

size_t gnca_step_tangent_workspace_bytes(const gnca_step_desc* desc) {
  TanLayout T;
  return tan_layout(desc, &T) ? T.bytes : 0;
}

// the body of gnca_step_tangent (dw == NULL) and of gnca_step_tangent_params
static int step_tangent_entry(const gnca_step_desc* desc, const gnca_weights* w, const gnca_weights* dw,
                              const float* x, const void* fire, const uint8_t* active, const float* v, float* x_out,
                              float* v_out, void* ws, size_t ws_bytes, void* hip_stream) {
  if (!desc || !w || !x || !v || !x_out || !v_out) return GNCA_ERR_INVALID;
  if (!outputs_distinct({x_out, v_out}, x, v, dw, 1)) return GNCA_ERR_INVALID;
  if (tangent_unsupported(desc)) return GNCA_ERR_UNSUPPORTED;
  TanLayout T;
  if (!tan_layout(desc, &T)) return outside_support(desc) ? GNCA_ERR_UNSUPPORTED : GNCA_ERR_INVALID;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  StreamDeviceGuard dg(st);
  return step_tangent_impl(desc, w, dw, x, fire, active, v, x_out, v_out, ws, ws_bytes, st);
}

int gnca_step_tangent(const gnca_step_desc* desc, const gnca_weights* w, const float* x, const void* fire,
                      const uint8_t* active, const float* v, float* x_out, float* v_out, void* ws, size_t ws_bytes,
                      void* hip_stream) {
  return step_tangent_entry(desc, w, nullptr, x, fire, active, v, x_out, v_out, ws, ws_bytes, hip_stream);
}

int gnca_step_tangent_params(const gnca_step_desc* desc, const gnca_weights* w, const gnca_weights* dw,
                             const float* x, const void* fire, const uint8_t* active, const float* v, float* x_out,
                             float* v_out, void* ws, size_t ws_bytes, void* hip_stream) {
  if (!dw) return GNCA_ERR_INVALID;
  return step_tangent_entry(desc, w, dw, x, fire, active, v, x_out, v_out, ws, ws_bytes, hip_stream);
}

size_t gnca_rollout_tangent_workspace_bytes(const gnca_step_desc* desc, const gnca_rollout_sched* sched,
                                            const gnca_tangent_args* args) {
  RollTanLayout L;
  if (!desc || !sched || !args) return 0;
  return roll_tan_layout(desc, sched, args, &L) ? L.bytes : 0;
}

// the body of gnca_rollout_tangent (dw == NULL) and of gnca_rollout_tangent_params
static int rollout_tangent_entry(const gnca_step_desc* desc, const gnca_weights* w, const gnca_weights* dw,
                                 const gnca_rollout_sched* sched, const gnca_tangent_args* args, const float* x,
                                 const float* v, float* x_final, float* v_final, void* ws, size_t ws_bytes) {
  if (!desc || !w || !sched || !args || !x || !v || !x_final || !v_final) return GNCA_ERR_INVALID;
  if (!outputs_distinct({x_final, v_final}, x, v, dw, 1)) return GNCA_ERR_INVALID;
  // rescaling v alone breaks linearity in the pair (v, dtheta)
  if (dw && (args->flags & GNCA_TANGENT_RENORM)) return GNCA_ERR_INVALID;
  if (!records_ok(sched, args) || (args->num_records > 0 && !args->log_norm)) return GNCA_ERR_INVALID;
  RollTanLayout L;
  const bool laid = roll_tan_layout(desc, sched, args, &L);
  int rc = tan_roll_check(desc, sched, false, laid, laid && ws && ws_bytes >= L.bytes);
  if (rc != GNCA_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(args->stream);
  StreamDeviceGuard dg(st);
  const int B = desc->B;
  const size_t n = (size_t)desc->C * desc->H * desc->W;
  char* wsb = reinterpret_cast<char*>(ws);
  double* pn = reinterpret_cast<double*>(wsb + L.off_pn);
  double* carry = reinterpret_cast<double*>(wsb + L.off_carry);
  float* scale = reinterpret_cast<float*>(wsb + L.off_scale);
  const TanRoll roll = {1, dw, x, v, x_final, v_final, nullptr, 0, 0, args->num_records > 0 ? carry : nullptr, B};
  int r = 0;
  return tangent_rollout(desc, w, sched, L.R, wsb, roll, st, [&](int t, float*, float* vn) {
    if (r >= args->num_records || args->record[r] != t + 1) return (int)GNCA_OK;
    const dim3 g((unsigned)L.nchunk, (unsigned)B);
    const int renorm = (args->flags & GNCA_TANGENT_RENORM) ? 1 : 0;
    hipLaunchKernelGGL(gnca_t_sumsq, g, dim3(kThreads), 0, st, (const float*)vn, pn, n, L.nchunk);
    if ((rc = t_check()) != GNCA_OK) return rc;
    hipLaunchKernelGGL(gnca_t_lognorm, dim3((unsigned)B), dim3(64), 0, st, (const double*)pn, L.nchunk, carry, scale,
                       args->log_norm + (size_t)r * B, renorm, 1);
    if ((rc = t_check()) != GNCA_OK) return rc;
    ++r;
    if (!renorm) return (int)GNCA_OK;
    hipLaunchKernelGGL(gnca_t_scale, g, dim3(kThreads), 0, st, vn, (const float*)scale, n);
    return t_check();
  });
}

int gnca_rollout_tangent(const gnca_step_desc* desc, const gnca_weights* w, const gnca_rollout_sched* sched,
                         const gnca_tangent_args* args, const float* x, const float* v, float* x_final,
                         float* v_final, void* ws, size_t ws_bytes) {
  return rollout_tangent_entry(desc, w, nullptr, sched, args, x, v, x_final, v_final, ws, ws_bytes);
}

int gnca_rollout_tangent_params(const gnca_step_desc* desc, const gnca_weights* w, const gnca_weights* dw,
                                const gnca_rollout_sched* sched, const gnca_tangent_args* args, const float* x,
                                const float* v, float* x_final, float* v_final, void* ws, size_t ws_bytes) {
  if (!dw) return GNCA_ERR_INVALID;
  return rollout_tangent_entry(desc, w, dw, sched, args, x, v, x_final, v_final, ws, ws_bytes);
}

size_t gnca_tangent_qr_workspace_bytes(int32_t num_dirs, int32_t B, int64_t n) {
  QrLayout Q;
  return qr_layout(num_dirs, B, n, &Q) ? Q.bytes : 0;
}

int gnca_tangent_qr(int32_t num_dirs, int32_t B, int64_t n, float* v, double* r, double* log_diag, void* ws,
                    size_t ws_bytes, void* hip_stream) {
  QrLayout Q;
  if (!v || !qr_layout(num_dirs, B, n, &Q)) return GNCA_ERR_INVALID;
  if (!ws || ws_bytes < Q.bytes) return GNCA_ERR_WORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  StreamDeviceGuard dg(st);
  return launch_qr(Q, num_dirs, B, (size_t)n, (size_t)B * (size_t)n, v, r, log_diag, nullptr,
                   reinterpret_cast<char*>(ws), st);
}

size_t gnca_rollout_tangent_block_workspace_bytes(const gnca_step_desc* desc, const gnca_rollout_sched* sched,
                                                  const gnca_tangent_block_args* args) {
  BlockTanLayout L;
  if (!desc || !sched || !args) return 0;
  return block_tan_layout(desc, sched, args, &L) ? L.bytes : 0;
}

// the body of gnca_rollout_tangent_block (dw == NULL) and of gnca_rollout_tangent_block_params (dw [K])
static int rollout_tangent_block_entry(const gnca_step_desc* desc, const gnca_weights* w, const gnca_weights* dw,
                                       const gnca_rollout_sched* sched, const gnca_tangent_block_args* args,
                                       const float* x, const float* v, float* x_final, float* v_final, void* ws,
                                       size_t ws_bytes) {
  if (!desc || !w || !sched || !args || !x || !v || !x_final || !v_final) return GNCA_ERR_INVALID;
  if (!block_records_ok(sched, args) || (args->num_records > 0 && !args->log_r)) return GNCA_ERR_INVALID;
  if (!outputs_distinct({x_final, v_final}, x, v, dw, args->num_dirs)) return GNCA_ERR_INVALID;
  // mixing the v_j alone breaks linearity in the pairs (v_j, dtheta_j)
  if (dw && (args->flags & GNCA_TBLOCK_ORTHO)) return GNCA_ERR_INVALID;
  BlockTanLayout L;
  const bool laid = block_tan_layout(desc, sched, args, &L);
  int rc = tan_roll_check(desc, sched, false, laid, laid && ws && ws_bytes >= L.bytes);
  if (rc != GNCA_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(args->stream);
  StreamDeviceGuard dg(st);
  const int B = desc->B, K = args->num_dirs;
  const size_t n = (size_t)desc->C * desc->H * desc->W, dstride = (size_t)B * n;
  char* wsb = reinterpret_cast<char*>(ws);
  double* pn = reinterpret_cast<double*>(wsb + L.off_pn);
  float* scale = reinterpret_cast<float*>(wsb + L.off_scale);
  double* carry = reinterpret_cast<double*>(wsb + L.off_carry);
  const bool ortho = (args->flags & GNCA_TBLOCK_ORTHO) != 0;
  // (without ORTHO the first B carries serve every direction and stay zero)
  const TanRoll roll = {K, dw, x, v, x_final, v_final, nullptr, 0, 0, args->num_records > 0 ? carry : nullptr, B * K};
  int r = 0;
  return tangent_rollout(desc, w, sched, L.R, wsb, roll, st, [&](int t, float*, float* vn) {
    if (r >= args->num_records || args->record[r] != t + 1) return (int)GNCA_OK;
    double* out = args->log_r + (size_t)r++ * B * K;
    if (ortho) return launch_qr(L.Q, K, B, n, dstride, vn, nullptr, out, carry, wsb + L.off_qr, st);
    for (int j = 0; j < K; ++j) {
      hipLaunchKernelGGL(gnca_t_sumsq, dim3((unsigned)L.nchunk, (unsigned)B), dim3(kThreads), 0, st,
                         (const float*)(vn + (size_t)j * dstride), pn, n, L.nchunk);
      if ((rc = t_check()) != GNCA_OK) return rc;
      hipLaunchKernelGGL(gnca_t_lognorm, dim3((unsigned)B), dim3(64), 0, st, (const double*)pn, L.nchunk, carry,
                         scale, out + j, 0, K);
      if ((rc = t_check()) != GNCA_OK) return rc;
    }
    return (int)GNCA_OK;
  });
}

int gnca_rollout_tangent_block(const gnca_step_desc* desc, const gnca_weights* w, const gnca_rollout_sched* sched,
                               const gnca_tangent_block_args* args, const float* x, const float* v,
                               float* x_final, float* v_final, void* ws, size_t ws_bytes) {
  return rollout_tangent_block_entry(desc, w, nullptr, sched, args, x, v, x_final, v_final, ws, ws_bytes);
}

int gnca_rollout_tangent_block_params(const gnca_step_desc* desc, const gnca_weights* w, const gnca_weights* dw,
                                      const gnca_rollout_sched* sched, const gnca_tangent_block_args* args,
                                      const float* x, const float* v, float* x_final, float* v_final, void* ws,
                                      size_t ws_bytes) {
  if (!dw) return GNCA_ERR_INVALID;
  return rollout_tangent_block_entry(desc, w, dw, sched, args, x, v, x_final, v_final, ws, ws_bytes);
}

size_t gnca_rollout_objective_tangent_workspace_bytes(const gnca_step_desc* desc, const gnca_rollout_sched* sched,
                                                      const gnca_rollout_taps* taps, int32_t num_dirs) {
  TanRollLayout R;
  if (!desc || !sched || !taps) return 0;
  return obj_tan_layout(desc, sched, taps, num_dirs, &R) ? R.bytes : 0;
}

// after a tapped step has written (xn, vn), gnca_tap_loss_tangent reads them in place
int gnca_rollout_objective_tangent(const gnca_step_desc* desc, const gnca_weights* w, const gnca_weights* dw,
                                   const gnca_rollout_sched* sched, const gnca_rollout_taps* taps, int32_t num_dirs,
                                   const float* x, const float* v, float* x_final, float* v_final, float* losses,
                                   double* dlosses, int32_t* alive_count, void* ws, size_t ws_bytes) {
  if (!desc || !w || !sched || !taps || !x || !x_final || !losses || !dlosses) return GNCA_ERR_INVALID;
  if (!v && !dw) return GNCA_ERR_INVALID;
  if (num_dirs < 1 || num_dirs > kMaxDirs) return GNCA_ERR_INVALID;
  if (!outputs_distinct({x_final, losses, dlosses, v_final, alive_count}, x, v, dw, num_dirs)) return GNCA_ERR_INVALID;
  if (!taps_ok(desc, sched, taps) || (taps->kind == GNCA_TAP_MASKED && !alive_count)) return GNCA_ERR_INVALID;
  TanRollLayout R;
  const bool laid = obj_tan_layout(desc, sched, taps, num_dirs, &R);
  const int rc = tan_roll_check(desc, sched, false, laid, laid && ws && ws_bytes >= R.bytes);
  if (rc != GNCA_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(taps->stream);
  StreamDeviceGuard dg(st);
  const int B = desc->B, K = num_dirs;   // (steps >= 1: a tap list is never empty)
  const size_t n = (size_t)desc->C * desc->H * desc->W, dstride = (size_t)B * n;
  const TanRoll roll = {K, dw, x, v, x_final, v_final, nullptr, 0, 0, nullptr, 0};
  int r = 0;
  return tangent_rollout(desc, w, sched, R, reinterpret_cast<char*>(ws), roll, st, [&](int t, float* xn, float* vn) {
    if (r >= taps->n || taps->steps[r] != t + 1) return (int)GNCA_OK;
    const int q = r++;
    return launch_tap_loss_tangent(taps->kind, &taps->masked, K, xn, n, vn, dstride, n, taps->target,
                                   (long)taps->target_bstride, losses + (size_t)q * B, dlosses + (size_t)q * K * B,
                                   q == 0 ? alive_count : nullptr, st);
  });
}

size_t gnca_rollout_gn_fwd_workspace_bytes(const gnca_step_desc* desc, const gnca_rollout_sched* sched,
                                           const gnca_rollout_taps* taps) {
  GnFwdLayout L;
  if (!desc || !sched || !taps) return 0;
  return gn_fwd_layout(desc, sched, taps, &L) ? L.R.bytes : 0;
}

// one direction, with the primal's states written where gnca_rollout_fwd_f32 writes them on a states-only tape;
// after a tapped step has written (xn, vn), gnca_tap_curvature reads them in place
int gnca_rollout_gn_fwd(const gnca_step_desc* desc, const gnca_weights* w, const gnca_weights* dw,
                        const gnca_rollout_sched* sched, const gnca_rollout_taps* taps, const float* x, const float* v,
                        float* x_final, void* tape, size_t tape_bytes, float* fields, float* losses, double* dlosses,
                        double* quad, int32_t* alive_count, void* ws, size_t ws_bytes) {
  if (!desc || !w || !sched || !taps || !x || !x_final || !tape || !fields || !losses || !dlosses || !quad)
    return GNCA_ERR_INVALID;
  if (!v && !dw) return GNCA_ERR_INVALID;
  if (!outputs_distinct({x_final, tape, fields, losses, dlosses, quad, alive_count}, x, v, dw, 1))
    return GNCA_ERR_INVALID;
  if (!taps_ok(desc, sched, taps) || (taps->kind == GNCA_TAP_MASKED && !alive_count)) return GNCA_ERR_INVALID;
  GnFwdLayout L;
  const bool laid = gn_fwd_layout(desc, sched, taps, &L);
  const int rc = tan_roll_check(desc, sched, true, laid,
                                laid && tape_bytes >= L.T.bytes && ws && ws_bytes >= L.R.bytes);
  if (rc != GNCA_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(taps->stream);
  StreamDeviceGuard dg(st);
  const int B = desc->B;   // (steps >= 1: a tap list is never empty)
  const size_t HW = (size_t)desc->H * desc->W, n = (size_t)desc->C * HW;
  const TanRoll roll = {1, dw, x, v, x_final, nullptr, reinterpret_cast<char*>(tape), L.T.slot, L.T.k, nullptr, 0};
  int r = 0;
  return tangent_rollout(desc, w, sched, L.R, reinterpret_cast<char*>(ws), roll, st, [&](int t, float* xn, float* vn) {
    if (r >= taps->n || taps->steps[r] != t + 1) return (int)GNCA_OK;
    const int q = r++;
    return launch_tap_curvature(taps->kind, &taps->masked, xn, n, vn, n, taps->target, (long)taps->target_bstride,
                                losses + (size_t)q * B, dlosses + (size_t)q * B, quad + (size_t)q * B,
                                fields + (size_t)q * B * 4 * HW, 4 * HW, q == 0 ? alive_count : nullptr, st);
  });
}

}  // extern "C"
