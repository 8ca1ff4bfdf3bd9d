// gnca_aux.hip — step-adjacent batch ops of the rollout/training loop:
// the damage curriculum (reference: src/utils/damage.py:15-138), one launch for the whole batch,
// the premultiplied-RGBA loss, the classic trainer's target-masked loss and stability loss, and the
// image metrics (mse, pixel-perfect, psnr, ssim).
//
// The reference loops over samples on the host, drawing each sample's position with a separate
// torch.randint(...).item()-style call (a device sync per sample on GPU) and applying a masked
// assignment per sample.  Here every sample's random draws arrive in device arrays and one
// elementwise kernel applies the damage to all of them.

#include "gnca_device.h"

namespace gnca {
namespace {

__global__ __launch_bounds__(kThreads) void gnca_damage(const gnca_damage_desc d, float* state,
                                                        const int32_t* pos, const float* noise) {
  const int C = d.C, H = d.H, W = d.W;
  const size_t HW = (size_t)H * W;
  const size_t cells = (size_t)d.B * HW;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < cells; e += (size_t)gridDim.x * kThreads) {
    const int b = (int)(e / HW);
    const size_t cell = e - (size_t)b * HW;
    const int i = (int)(cell / W), j = (int)(cell - (size_t)i * W);
    float* sb = state + (size_t)b * C * HW + cell;
    const int py = pos ? pos[2 * b] : 0, px = pos ? pos[2 * b + 1] : 0;
    const int sz = d.size;
    switch (d.kind) {
      case GNCA_DMG_SQUARE:        // damage.py:15-23
        if (i >= py && i < py + sz && j >= px && j < px + sz)
          for (int c = 0; c < C; ++c) sb[c * HW] = 0.f;
        break;
      case GNCA_DMG_CIRCLE: {      // damage.py:25-36 (float compare, as the reference)
        const float dy = (float)i - (float)py, dx = (float)j - (float)px;
        if (dy * dy + dx * dx <= (float)(sz * sz))
          for (int c = 0; c < C; ++c) sb[c * HW] = 0.f;
        break;
      }
      case GNCA_DMG_STRIPE_H:      // damage.py:38-50
        if (i >= py && i < py + sz)
          for (int c = 0; c < C; ++c) sb[c * HW] = 0.f;
        break;
      case GNCA_DMG_STRIPE_V:
        if (j >= px && j < px + sz)
          for (int c = 0; c < C; ++c) sb[c * HW] = 0.f;
        break;
      case GNCA_DMG_ALPHA_DROP:    // damage.py:52-65, hard: state *= (1 - drop)
      case GNCA_DMG_ALPHA_DROP_SOFT: {
        const float a = sb[3 * HW];
        const float drop = (noise[(size_t)b * HW + cell] < d.p ? 1.f : 0.f) * (a > d.alpha_thr ? 1.f : 0.f);
        if (d.kind == GNCA_DMG_ALPHA_DROP) {
          for (int c = 0; c < C; ++c) sb[c * HW] *= (1.f - drop);
        } else {
          sb[3 * HW] = a * (1.f - drop);
        }
        break;
      }
      case GNCA_DMG_SALT_PEPPER:   // damage.py:67-72
        sb[3 * HW] *= (1.f - (noise[(size_t)b * HW + cell] < d.p ? 1.f : 0.f));
        break;
      case GNCA_DMG_GAUSSIAN: {    // damage.py:82-97
        const float dy = (float)i - (float)py, dx = (float)j - (float)px;
        const float r2 = dy * dy + dx * dx;
        const float s = (float)sz * fmaxf(1e-6f, d.softness);
        const float m = expf(-(r2 / (2.f * s * s)));
        const float damp = fminf(fmaxf(1.f - m, 0.f), 1.f);
        for (int c = 0; c < C; ++c) sb[c * HW] *= damp;
        break;
      }
      case GNCA_DMG_HIDDEN_NOISE:  // damage.py:74-80
        for (int c = 4; c < C; ++c) {
          const float v = sb[c * HW] + noise[((size_t)b * (C - 4) + (c - 4)) * HW + cell] * d.sigma;
          sb[c * HW] = fminf(fmaxf(v, 0.f), 1.f);
        }
        break;
      default:
        break;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The damage policy with its draws on the device (gnca_damage_policy; include/gnca.h holds the
// RNG's definition and the draw rules).  Per cell the arithmetic is gnca_damage's above, kept in
// step with it expression by expression: tests/test_gpu_damage_policy.py compares the two bitwise.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t dmg_key(uint64_t k1, uint64_t sample, int stream) {
  return mix64(k1 ^ ((sample << 8) | (uint64_t)stream));
}

__device__ __forceinline__ uint32_t dmg_draw(uint64_t k2, uint64_t index) {
  return (uint32_t)(mix64(k2 + index) >> 40);
}

__device__ __forceinline__ float dmg_uniform(uint32_t d) { return (float)d * (1.0f / 16777216.0f); }

// integer in [lo, hi] (hi >= lo)
__device__ __forceinline__ int dmg_randint(uint32_t d, int lo, int hi) {
  return lo + (int)(((uint64_t)d * (uint64_t)((int64_t)hi - lo + 1)) >> 24);
}

__device__ __forceinline__ float dmg_normal(uint32_t d1, uint32_t d2) {
  const float u1 = (float)(d1 + 1u) * (1.0f / 16777216.0f);
  const float u2 = (float)d2 * (1.0f / 16777216.0f);
  return sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// One sample's scalar draws: (applied, primitive kind, size argument, y, x) are gnca_damage's kind,
// size and pos[b].  Depends on the workgroup's sample only, so it stays on the scalar unit.
struct DmgDraws {
  int applied, prim, arg, y, x;
};

__device__ __forceinline__ DmgDraws dmg_sample_draws(const gnca_damage_policy_desc& d, uint64_t k1, int b,
                                                     const int32_t* forced) {
  DmgDraws s = {0, -1, 0, 0, 0};
  const uint64_t gs = (uint64_t)(d.sample_base + b);
  const bool per_sample = d.scope == GNCA_DMG_SCOPE_SAMPLE;
  const uint64_t ks = per_sample ? gs : GNCA_DMG_SHARED_SAMPLE;   // the key of the scalar draws
  int kind = -1;
  if (forced != nullptr) {
    kind = forced[b];
    if (kind < GNCA_DMG_SQUARE || kind > GNCA_DMG_STRIPES_AUTO) return s;
  } else {
    if (!(dmg_uniform(dmg_draw(dmg_key(k1, GNCA_DMG_SHARED_SAMPLE, GNCA_DMG_RNG_GATE), 0)) <= d.prob)) return s;
    if (per_sample && !(dmg_uniform(dmg_draw(dmg_key(k1, gs, GNCA_DMG_RNG_SAMPLE_GATE), 0)) <= d.per_sample_prob))
      return s;
    const float uk = dmg_uniform(dmg_draw(dmg_key(k1, ks, GNCA_DMG_RNG_KIND), 0));
#pragma unroll
    for (int k = GNCA_DMG_MAX_KINDS - 1; k >= 0; --k)   // ends on the smallest k with uk < cum[k]
      if (k < d.n_kinds && (uk < d.cum[k] || k == d.n_kinds - 1)) kind = d.kinds[k];
  }
  const int size = dmg_randint(dmg_draw(dmg_key(k1, ks, GNCA_DMG_RNG_SIZE), 0), d.size_min, d.size_max);
  const int H = d.H, W = d.W;
  switch (kind) {
    case GNCA_DMG_SQUARE:
      if (size <= 0) return s;
      s.arg = size;
      s.y = dmg_randint(dmg_draw(dmg_key(k1, gs, GNCA_DMG_RNG_Y), 0), 0, max(1, H - size + 1) - 1);
      s.x = dmg_randint(dmg_draw(dmg_key(k1, gs, GNCA_DMG_RNG_X), 0), 0, max(1, W - size + 1) - 1);
      break;
    case GNCA_DMG_CIRCLE:
    case GNCA_DMG_GAUSSIAN: {
      const int r = size > 1 ? size / 2 : 1;
      s.arg = r;
      s.y = dmg_randint(dmg_draw(dmg_key(k1, gs, GNCA_DMG_RNG_Y), 0), r, max(r + 1, H - r) - 1);
      s.x = dmg_randint(dmg_draw(dmg_key(k1, gs, GNCA_DMG_RNG_X), 0), r, max(r + 1, W - r) - 1);
      break;
    }
    case GNCA_DMG_STRIPE_H:
    case GNCA_DMG_STRIPE_V:
    case GNCA_DMG_STRIPES_AUTO: {
      const int width = d.stripe_width > 0 ? d.stripe_width : size;
      if (width <= 0) return s;
      s.arg = width;
      if (kind == GNCA_DMG_STRIPES_AUTO)
        kind = dmg_draw(dmg_key(k1, ks, GNCA_DMG_RNG_ORIENT), 0) < (1u << 23) ? GNCA_DMG_STRIPE_H : GNCA_DMG_STRIPE_V;
      if (kind == GNCA_DMG_STRIPE_H)
        s.y = dmg_randint(dmg_draw(dmg_key(k1, ks, GNCA_DMG_RNG_Y), 0), 0, max(1, H - width + 1) - 1);
      else
        s.x = dmg_randint(dmg_draw(dmg_key(k1, ks, GNCA_DMG_RNG_X), 0), 0, max(1, W - width + 1) - 1);
      break;
    }
    case GNCA_DMG_ALPHA_DROP:
    case GNCA_DMG_ALPHA_DROP_SOFT:
      if (d.alpha_dropout_p <= 0.f) return s;
      break;
    case GNCA_DMG_SALT_PEPPER:
      if (d.salt_pepper_p <= 0.f) return s;
      break;
    case GNCA_DMG_HIDDEN_NOISE:
      if (d.C <= 4 || d.hidden_sigma <= 0.f) return s;
      break;
    default:
      return s;
  }
  s.applied = 1;
  s.prim = kind;
  return s;
}

__host__ __device__ inline int dmg_clampi(long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

// Workgroup (band, sample): rows [band * band_rows, ...) of sample blockIdx.x / nbands.  V = 4: 16-byte
// accesses along W (W % 4 == 0 and 16-byte aligned bases), V = 1 otherwise.  Only the rows and vector
// columns of the kind's bounding box are visited; a multiplicative kind reads and writes only the
// vectors that hold a cell whose factor is not 1, and changes only those cells.
template <int V>
__global__ __launch_bounds__(kThreads) void gnca_damage_policy_k(const gnca_damage_policy_desc d, int band_rows,
                                                                 int nbands, float* state, const int32_t* forced,
                                                                 const int64_t* event_dev, int32_t* draws_out,
                                                                 float* noise_out) {
  typedef float vf __attribute__((ext_vector_type(V)));
  const int tid = threadIdx.x;
  const int b = (int)(blockIdx.x / (unsigned)nbands), band = (int)(blockIdx.x % (unsigned)nbands);
  const int C = d.C, H = d.H, W = d.W;
  const size_t HW = (size_t)H * W;
  const int64_t event = event_dev != nullptr ? event_dev[0] : d.event;
  const uint64_t k0 = mix64(d.seed + 0xD6E8FEB86659FD93ull);
  const uint64_t k1 = mix64(k0 + 0x9E3779B97F4A7C15ull * (uint64_t)(event + 1));
  const DmgDraws s = dmg_sample_draws(d, k1, b, forced);
  if (band == 0 && draws_out != nullptr && tid < 8) {
    const int v = tid == 0 ? s.applied : tid == 1 ? s.prim : tid == 2 ? s.arg : tid == 3 ? s.y : tid == 4 ? s.x : 0;
    draws_out[(size_t)8 * b + tid] = v;
  }
  if (!s.applied) return;

  // the kind's bounding box [y0, y1) x [x0, x1), clipped to the field
  const int sz = s.arg, py = s.y, px = s.x;
  long y0 = 0, y1 = H, x0 = 0, x1 = W;
  switch (s.prim) {
    case GNCA_DMG_SQUARE:   y0 = py; y1 = (long)py + sz; x0 = px; x1 = (long)px + sz; break;
    case GNCA_DMG_CIRCLE:   y0 = (long)py - sz; y1 = (long)py + sz + 1; x0 = (long)px - sz; x1 = (long)px + sz + 1; break;
    case GNCA_DMG_STRIPE_H: y0 = py; y1 = (long)py + sz; break;
    case GNCA_DMG_STRIPE_V: x0 = px; x1 = (long)px + sz; break;
    case GNCA_DMG_GAUSSIAN: {
      // damp = 1 - exp(-r2 / (2 s^2)) rounds to 1 once the exponent passes 25 ln 2 = 17.33: outside
      // |dy|, |dx| <= 6 s + 2 (exponent > 18) every factor is exactly 1
      const float ext = 6.f * ((float)sz * fmaxf(1e-6f, d.gaussian_softness)) + 2.f;
      if (ext < 1e9f) {
        const long e = (long)ext;
        y0 = (long)py - e; y1 = (long)py + e + 1; x0 = (long)px - e; x1 = (long)px + e + 1;
      }
      break;
    }
    default: break;
  }
  const int r0 = band * band_rows;
  const int lo = max(r0, dmg_clampi(y0, 0, H)), hi = min(min(r0 + band_rows, H), dmg_clampi(y1, 0, H));
  const int cx0 = dmg_clampi(x0, 0, W), cx1 = dmg_clampi(x1, 0, W);
  if (lo >= hi || cx0 >= cx1) return;
  const int vx0 = cx0 / V, nvx = (cx1 + V - 1) / V - vx0;
  const int total = (hi - lo) * nvx;

  const uint64_t gsmp = (uint64_t)(d.sample_base + b);
  const uint64_t kc = dmg_key(k1, gsmp, GNCA_DMG_RNG_CELL);
  const uint64_t kn1 = dmg_key(k1, gsmp, GNCA_DMG_RNG_NORMAL_U1), kn2 = dmg_key(k1, gsmp, GNCA_DMG_RNG_NORMAL_U2);
  const int NP = C > 4 ? C - 4 : 1;
  float* sample = state + (size_t)b * C * HW;
  float* nz = noise_out != nullptr ? noise_out + (size_t)b * NP * HW : nullptr;

  for (int t = tid; t < total; t += kThreads) {
    const int i = lo + t / nvx, j0 = (vx0 + t % nvx) * V;
    const size_t cell = (size_t)i * W + j0;
    float* sb = sample + cell;
    switch (s.prim) {
      case GNCA_DMG_SQUARE:
      case GNCA_DMG_CIRCLE:
      case GNCA_DMG_STRIPE_H:
      case GNCA_DMG_STRIPE_V: {
        bool in[V];
        int n = 0;
#pragma unroll
        for (int l = 0; l < V; ++l) {
          const int j = j0 + l;
          if (s.prim == GNCA_DMG_SQUARE) {
            in[l] = i >= py && i < py + sz && j >= px && j < px + sz;
          } else if (s.prim == GNCA_DMG_CIRCLE) {
            const float dy = (float)i - (float)py, dx = (float)j - (float)px;
            in[l] = dy * dy + dx * dx <= (float)(sz * sz);
          } else if (s.prim == GNCA_DMG_STRIPE_H) {
            in[l] = i >= py && i < py + sz;
          } else {
            in[l] = j >= px && j < px + sz;
          }
          n += in[l] ? 1 : 0;
        }
        if (n == V) {
          vf z;
#pragma unroll
          for (int l = 0; l < V; ++l) z[l] = 0.f;
          for (int c = 0; c < C; ++c) *reinterpret_cast<vf*>(sb + c * HW) = z;
        } else if (n > 0) {
#pragma unroll
          for (int l = 0; l < V; ++l)
            if (in[l])
              for (int c = 0; c < C; ++c) sb[c * HW + l] = 0.f;
        }
        break;
      }
      case GNCA_DMG_GAUSSIAN: {
        float f[V];
        bool any = false;
#pragma unroll
        for (int l = 0; l < V; ++l) {
          const float dy = (float)i - (float)py, dx = (float)(j0 + l) - (float)px;
          const float r2 = dy * dy + dx * dx;
          const float sg = (float)sz * fmaxf(1e-6f, d.gaussian_softness);
          const float m = expf(-(r2 / (2.f * sg * sg)));
          f[l] = fminf(fmaxf(1.f - m, 0.f), 1.f);
          any = any || f[l] != 1.f;
        }
        if (!any) break;
        for (int c = 0; c < C; ++c) {
          vf x = *reinterpret_cast<const vf*>(sb + c * HW);
#pragma unroll
          for (int l = 0; l < V; ++l)
            if (f[l] != 1.f) x[l] *= f[l];
          *reinterpret_cast<vf*>(sb + c * HW) = x;
        }
        break;
      }
      case GNCA_DMG_ALPHA_DROP:
      case GNCA_DMG_ALPHA_DROP_SOFT:
      case GNCA_DMG_SALT_PEPPER: {
        const float p = s.prim == GNCA_DMG_SALT_PEPPER ? d.salt_pepper_p : d.alpha_dropout_p;
        vf u;
        bool hit[V];
        bool any = false;
#pragma unroll
        for (int l = 0; l < V; ++l) {
          u[l] = dmg_uniform(dmg_draw(kc, cell + l));
          hit[l] = u[l] < p;
          any = any || hit[l];
        }
        if (nz != nullptr) *reinterpret_cast<vf*>(nz + cell) = u;
        if (!any) break;
        vf a = *reinterpret_cast<const vf*>(sb + 3 * HW);
        if (s.prim == GNCA_DMG_SALT_PEPPER) {
#pragma unroll
          for (int l = 0; l < V; ++l)
            if (hit[l]) a[l] *= 0.f;   // (1 - 1): the sign of zero kept
          *reinterpret_cast<vf*>(sb + 3 * HW) = a;
          break;
        }
        any = false;
#pragma unroll
        for (int l = 0; l < V; ++l) {
          hit[l] = hit[l] && a[l] > d.alpha_thr;
          any = any || hit[l];
        }
        if (!any) break;
        if (s.prim == GNCA_DMG_ALPHA_DROP) {   // hard: every channel *= (1 - drop), the sign of zero kept
          for (int c = 0; c < C; ++c) {
            vf x = *reinterpret_cast<const vf*>(sb + c * HW);
#pragma unroll
            for (int l = 0; l < V; ++l)
              if (hit[l]) x[l] *= 0.f;
            *reinterpret_cast<vf*>(sb + c * HW) = x;
          }
        } else {
#pragma unroll
          for (int l = 0; l < V; ++l)
            if (hit[l]) a[l] = a[l] * 0.f;
          *reinterpret_cast<vf*>(sb + 3 * HW) = a;
        }
        break;
      }
      case GNCA_DMG_HIDDEN_NOISE:
        for (int c = 4; c < C; ++c) {
          vf x = *reinterpret_cast<const vf*>(sb + c * HW);
          vf nn;
          const uint64_t idx = (uint64_t)(c - 4) * HW + cell;
#pragma unroll
          for (int l = 0; l < V; ++l) {
            nn[l] = dmg_normal(dmg_draw(kn1, idx + l), dmg_draw(kn2, idx + l));
            const float v = x[l] + nn[l] * d.hidden_sigma;
            x[l] = fminf(fmaxf(v, 0.f), 1.f);
          }
          *reinterpret_cast<vf*>(sb + c * HW) = x;
          if (nz != nullptr) *reinterpret_cast<vf*>(nz + idx) = nn;
        }
        break;
      default:
        break;
    }
  }
}

// loss_premult_rgba (train_graph_augmented_nca.py:52-61): one workgroup per sample, fixed-order
// fp64 reduction (deterministic).  The per-sample body, shared with gnca_tap_loss: the value is
// returned in thread 0 (red: one slot per wave).
__device__ __forceinline__ float premult_loss_sample(int H, int W, const float* p, const float* t, double* red) {
  const int tid = threadIdx.x;
  const size_t HW = (size_t)H * W;
  double acc = 0.0;
  for (size_t e = tid; e < HW; e += kThreads) {
    const float a = p[3 * HW + e];
    float s = 0.f;
    for (int c = 0; c < 3; ++c) {
      const float r = p[c * HW + e] * a - t[c * HW + e];
      s = fmaf(r, r, s);
    }
    const float ra = a - t[3 * HW + e];
    acc += (double)fmaf(ra, ra, s);
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  double v = 0.0;
  if (tid == 0) {
    for (int w = 0; w < kThreads / 64; ++w) v += red[w];
    v = v / (4.0 * (double)HW);
  }
  return (float)v;
}

__global__ __launch_bounds__(kThreads) void gnca_loss_fwd(int H, int W, const float* pred, long pbs,
                                                          const float* tgt, long tbs, float* out) {
  __shared__ double red[kThreads / 64];
  const int b = blockIdx.x;
  const float v = premult_loss_sample(H, W, pred + (size_t)b * pbs, tgt + (size_t)b * tbs, red);
  if (threadIdx.x == 0) out[b] = v;
}

// g * d loss_premult / d pred at cell q of one sample: the four channel values, in fp32.  Shared
// with gnca_tap_inject.
__device__ __forceinline__ void premult_grad_cell(size_t HW, const float* p, const float* t, size_t q, float g,
                                                  float v[4]) {
  const float s = g * (float)(2.0 / (4.0 * (double)HW));
  const float a = p[3 * HW + q];
  float ga = a - t[3 * HW + q];
  for (int c = 0; c < 3; ++c) {
    const float x = p[c * HW + q];
    const float r = x * a - t[c * HW + q];
    v[c] = s * r * a;
    ga = fmaf(r, x, ga);
  }
  v[3] = s * ga;
}

__global__ __launch_bounds__(kThreads) void gnca_loss_bwd(int B, int H, int W, const float* pred, long pbs,
                                                          const float* tgt, long tbs, const float* g,
                                                          float* gp, long gbs) {
  const size_t HW = (size_t)H * W, total = (size_t)B * HW;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (size_t)gridDim.x * kThreads) {
    const size_t b = e / HW, q = e - b * HW;
    float* o = gp + b * gbs;
    float v[4];
    premult_grad_cell(HW, pred + b * pbs, tgt + b * tbs, q, g[b], v);
    for (int c = 0; c < 4; ++c) o[c * HW + q] = v[c];
  }
}

// ---------------------------------------------------------------------------------------------
// The classic trainer's objective (train_intermediate_loss.py:37-51 and :256-267, with the graph
// trainer's two background penalties, train_graph_augmented_nca.py:30-49): MSE over the cells where
// the TARGET is alive plus three penalties, and the stability phase's MSE over the close samples.
// Both read 8 planes once (traffic- and latency-bound); every sum is a fixed-order fp64 sum (per
// thread, xor-shuffle, waves in order), so a sample's value does not depend on the batch around it.
// ---------------------------------------------------------------------------------------------

// the sum of `v` over the workgroup, in a fixed order, in every thread (red: one slot per wave)
__device__ inline double block_sum(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();   // (red may still be read from the previous sum)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < kThreads / 64; ++w) s += red[w];
  return s;
}

// The per-sample body of the masked loss, shared with gnca_tap_loss: every thread returns the value
// and the alive count (block_sum leaves each sum in all threads); thread 0 of the caller stores them.
__device__ __forceinline__ float masked_loss_sample(const gnca_masked_loss_desc& d, const float* p, const float* t,
                                                    double* red, int32_t* count) {
  const int tid = threadIdx.x;
  const size_t HW = (size_t)d.H * d.W;
  double prim = 0.0, bga = 0.0, bgrgb = 0.0, area = 0.0, cnt = 0.0;
  for (size_t e = tid; e < HW; e += kThreads) {
    const float ta = t[3 * HW + e], pa = p[3 * HW + e];
    const bool alive = ta > d.alpha_thr;
    area += (double)pa;
    if (alive) {
      cnt += 1.0;
      const float ra = pa - ta;
      prim += (double)(ra * ra);
      for (int c = 0; c < 3; ++c) {
        const float r = p[c * HW + e] - t[c * HW + e];   // the reference's fp32 difference, then its square
        prim += (double)(r * r);
      }
    } else {
      bga += (double)pa;
      for (int c = 0; c < 3; ++c) bgrgb += (double)fabsf(p[c * HW + e]);
    }
  }
  prim = block_sum(prim, red);
  bga = block_sum(bga, red);
  bgrgb = block_sum(bgrgb, red);
  area = block_sum(area, red);
  cnt = block_sum(cnt, red);   // (integers below 2^53: exact)
  const double hw = (double)HW;
  const double v = prim / (cnt + 1e-8) + (double)d.lam_bg_alpha * bga / hw +
                   (double)d.lam_bg_rgb * bgrgb / (3.0 * hw) + (double)d.lam_area * area / hw;
  *count = (int32_t)cnt;
  return (float)v;
}

__global__ __launch_bounds__(kThreads) void gnca_masked_loss_fwd(const gnca_masked_loss_desc d, const float* pred,
                                                                 long pbs, const float* tgt, long tbs, float* out,
                                                                 int32_t* alive_count, int32_t* nsteps_out) {
  __shared__ double red[kThreads / 64];
  const int b = blockIdx.x;
  int32_t cnt;
  const float vf = masked_loss_sample(d, pred + (size_t)b * pbs, tgt + (size_t)b * tbs, red, &cnt);
  if (threadIdx.x == 0) {
    out[b] = vf;
    alive_count[b] = cnt;
    if (nsteps_out) nsteps_out[b] = vf < d.close_thresh ? d.close_steps : 0;
  }
}

// g * d masked_loss / d pred at cell q of one sample (n: its alive count): the four channel values, in
// fp32.  Shared with gnca_tap_inject.
__device__ __forceinline__ void masked_grad_cell(const gnca_masked_loss_desc& d, size_t HW, const float* p,
                                                 const float* t, size_t q, float g, int32_t n, float v[4]) {
  const double hw = (double)HW;
  const double gb = (double)g;
  const float s = (float)(2.0 * gb / ((double)n + 1e-8));   // (unused where nothing is alive)
  const float ta = t[3 * HW + q], pa = p[3 * HW + q];
  const bool alive = ta > d.alpha_thr;
  const float pen_a = (float)(gb * ((alive ? 0.0 : (double)d.lam_bg_alpha) + (double)d.lam_area) / hw);
  const float pen_c = alive ? 0.f : (float)(gb * (double)d.lam_bg_rgb / (3.0 * hw));
  for (int c = 0; c < 3; ++c) {
    const float x = p[c * HW + q];
    const float sg = x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);   // torch's abs gradient: sign(0) = 0
    v[c] = alive ? s * (x - t[c * HW + q]) : pen_c * sg;
  }
  v[3] = alive ? fmaf(s, pa - ta, pen_a) : pen_a;
}

__global__ __launch_bounds__(kThreads) void gnca_masked_loss_bwd(const gnca_masked_loss_desc d, const float* pred,
                                                                 long pbs, const float* tgt, long tbs,
                                                                 const int32_t* alive_count, const float* g,
                                                                 float* gp, long gbs) {
  const size_t HW = (size_t)d.H * d.W, total = (size_t)d.B * HW;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (size_t)gridDim.x * kThreads) {
    const size_t b = e / HW, q = e - b * HW;
    float* o = gp + b * gbs;
    float v[4];
    masked_grad_cell(d, HW, pred + b * pbs, tgt + b * tbs, q, g[b], alive_count[b], v);
    for (int c = 0; c < 4; ++c) o[c * HW + q] = v[c];
  }
}

// ---------------------------------------------------------------------------------------------
// Taps: the two losses above on intermediate states of a rollout, read from its tape in place
// (gnca_rollout_tap_loss), and their gradients added to the backward's running cotangent
// (gnca_rollout_bwd_taps; the host loop is in gnca_bwd.hip).  Both kernels read 8 planes of
// a state once, threads along the cells of a plane (coalesced), and are traffic-bound.
// ---------------------------------------------------------------------------------------------
struct TapChunk {
  int first;                  // index r of the chunk's first tap
  int step[GNCA_TAP_CHUNK];   // the tapped step of each tap of the chunk (grid.y of them are read)
};

struct TapLossArgs {
  gnca_masked_loss_desc m;    // B, H, W (and the knobs of the masked kind)
  int T;
  const char* tape;
  size_t slot;                // bytes between two tape slots
  size_t sstride;             // a state's sample stride, C*H*W floats
  const float* x_final;       // the state after step T (not on the tape)
  const float* tgt;
  long tbs;
  float* losses;              // [R][B]
  int32_t* alive_count;       // [B], masked only
};

// grid (B, taps of the chunk): one workgroup per (tap, sample)
template <int KIND>
__global__ __launch_bounds__(kThreads) void gnca_tap_loss(const TapLossArgs a, const TapChunk ch) {
  __shared__ double red[kThreads / 64];
  const int b = blockIdx.x, r = ch.first + (int)blockIdx.y, t = ch.step[blockIdx.y];
  const float* state = t == a.T ? a.x_final : reinterpret_cast<const float*>(a.tape + (size_t)t * a.slot);
  const float* p = state + (size_t)b * a.sstride;
  const float* tg = a.tgt + (size_t)b * a.tbs;
  if (KIND == GNCA_TAP_PREMULT) {
    const float v = premult_loss_sample(a.m.H, a.m.W, p, tg, red);
    if (threadIdx.x == 0) a.losses[(size_t)r * a.m.B + b] = v;
  } else {
    int32_t cnt;
    const float v = masked_loss_sample(a.m, p, tg, red, &cnt);
    if (threadIdx.x == 0) {
      a.losses[(size_t)r * a.m.B + b] = v;
      if (r == 0) a.alive_count[b] = cnt;   // (the target's alone: the same at every tap)
    }
  }
}

// one rounded fp32 add: the pragma keeps it out of an FMA with the product that feeds it
__device__ __forceinline__ float add_rn(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}

struct TapInjectArgs {
  gnca_masked_loss_desc m;
  int C;
  const float* state;         // S_t [B,C,H,W]
  const float* tgt;
  long tbs;
  const int32_t* alive_count;
  const float* gl;            // g_losses[r] [B]
  const float* src;           // FULL: the cotangent the gradient is added to, or null (zeros)
  float* dst;                 // [B,C,H,W]
};

// one thread per cell (b, q).  !FULL: dst[b, c<4, q] += v.  FULL: every channel of dst is written,
// src + v on channels 0..3 and src on the rest (src == null: v and zeros).
template <int KIND, bool FULL>
__global__ __launch_bounds__(kThreads) void gnca_tap_inject(const TapInjectArgs a) {
  const size_t HW = (size_t)a.m.H * a.m.W, total = (size_t)a.m.B * HW, ss = (size_t)a.C * HW;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (size_t)gridDim.x * kThreads) {
    const size_t b = e / HW, q = e - b * HW;
    const float* p = a.state + b * ss;
    const float* tg = a.tgt + b * a.tbs;
    float v[4];
    if (KIND == GNCA_TAP_PREMULT) premult_grad_cell(HW, p, tg, q, a.gl[b], v);
    else masked_grad_cell(a.m, HW, p, tg, q, a.gl[b], a.alive_count[b], v);
    float* o = a.dst + b * ss + q;
    if (!FULL) {
      for (int c = 0; c < 4; ++c) o[c * HW] = add_rn(o[c * HW], v[c]);
    } else if (a.src != nullptr) {
      const float* s = a.src + b * ss + q;
      for (int c = 0; c < 4; ++c) o[c * HW] = add_rn(s[c * HW], v[c]);
      for (int c = 4; c < a.C; ++c) o[c * HW] = s[c * HW];
    } else {
      for (int c = 0; c < 4; ++c) o[c * HW] = v[c];
      for (int c = 4; c < a.C; ++c) o[c * HW] = 0.f;
    }
  }
}

// The forward-mode twin of gnca_tap_loss + gnca_tap_inject: the loss of one tapped
// state and its directional derivatives along K tangents of that state.
constexpr int kLossTanDirs = GNCA_LOSS_TANGENT_DIRS;

struct TapLossTanArgs {
  gnca_masked_loss_desc m;    // B, H, W (and the knobs of the masked kind)
  int K;
  const float* state;         // [B][>= 4][H][W], samples sstride floats apart
  size_t sstride;
  const float* tgt;
  long tbs;
  const float* v;             // direction k of sample b at v + k vds + b vbs, planes H*W apart
  size_t vds, vbs;
  float* losses;              // [B] of this tap, or null
  double* dlosses;            // [K][B] of this tap
  int32_t* alive_count;       // [B] or null (masked only)
};

// grid (B, ceil(K / kLossTanDirs)): one workgroup per (sample, chunk of directions).  The loss and, for the
// masked kind, the alive count come from the per-sample bodies above (chunk 0 stores them); then every thread
// takes the gradient's four values of each of its cells once, in registers, and multiplies them into the
// chunk's directions: one fp64 accumulator per direction, cells in the thread's order, channels ascending,
// then block_sum.  A direction's sum does not depend on its slot in the chunk, so not on K.
template <int KIND>
__global__ __launch_bounds__(kThreads) void gnca_tap_loss_tangent(const TapLossTanArgs a) {
  __shared__ double red[kThreads / 64];
  const int tid = threadIdx.x, b = blockIdx.x, k0 = (int)blockIdx.y * kLossTanDirs;
  const size_t HW = (size_t)a.m.H * a.m.W;
  const float* p = a.state + (size_t)b * a.sstride;
  const float* tg = a.tgt + (size_t)b * a.tbs;
  int32_t cnt = 0;
  if (KIND == GNCA_TAP_PREMULT) {
    if (blockIdx.y == 0 && a.losses != nullptr) {   // (uniform over the workgroup)
      const float l = premult_loss_sample(a.m.H, a.m.W, p, tg, red);
      if (tid == 0) a.losses[b] = l;
    }
  } else {
    const float l = masked_loss_sample(a.m, p, tg, red, &cnt);   // (every chunk needs the count)
    if (tid == 0 && blockIdx.y == 0) {
      if (a.losses != nullptr) a.losses[b] = l;
      if (a.alive_count != nullptr) a.alive_count[b] = cnt;
    }
  }
  const int nk = a.K - k0 < kLossTanDirs ? a.K - k0 : kLossTanDirs;
  const float* vb = a.v + (size_t)k0 * a.vds + (size_t)b * a.vbs;
  double acc[kLossTanDirs];
#pragma unroll
  for (int j = 0; j < kLossTanDirs; ++j) acc[j] = 0.0;
  for (size_t q = tid; q < HW; q += kThreads) {
    float g[4];
    if (KIND == GNCA_TAP_PREMULT) premult_grad_cell(HW, p, tg, q, 1.f, g);
    else masked_grad_cell(a.m, HW, p, tg, q, 1.f, cnt, g);
#pragma unroll
    for (int j = 0; j < kLossTanDirs; ++j)
      if (j < nk) {
        const float* vj = vb + (size_t)j * a.vds + q;
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[j] += (double)g[c] * (double)vj[c * HW];   // (the product is exact)
      }
  }
#pragma unroll
  for (int j = 0; j < kLossTanDirs; ++j)
    if (j < nk) {   // (uniform over the workgroup)
      const double s = block_sum(acc[j], red);
      if (tid == 0) a.dlosses[(size_t)(k0 + j) * a.m.B + b] = s;
    }
}

// The Gauss-Newton twin of gnca_tap_loss_tangent: the loss of one tapped state, its
// derivative along ONE tangent v of that state, and the loss's Gauss-Newton curvature applied to v and pulled
// back to the state: field = P^T H P v on channels 0..3, with quad = v^T P^T H P v.
struct TapCurvArgs {
  gnca_masked_loss_desc m;    // B, H, W (and the knobs of the masked kind)
  const float* state;         // [B][>= 4][H][W], samples sstride floats apart
  size_t sstride;
  const float* tgt;
  long tbs;
  const float* v;             // the tangent of sample b at v + b vbs, planes H*W apart
  size_t vbs;
  float* losses;              // [B] of this tap, or null
  double* dlosses;            // [B] of this tap, or null
  double* quad;               // [B] of this tap
  float* field;               // sample b at field + b fbs, four planes H*W apart
  size_t fbs;
  int32_t* alive_count;       // [B] or null (masked only)
};

// The four field values of one cell, each an fp64 expression of the fp32 inputs, and the cell's share of the
// quadratic form before its (2/N) factor.  No contraction: the expressions are the ones written here.
__device__ __forceinline__ double premult_curv_cell(size_t HW, const float* p, const float* v, size_t q, double s,
                                                    double f[4]) {
#pragma clang fp contract(off)
  const double a = (double)p[3 * HW + q], v3 = (double)v[3 * HW + q];
  double fa = v3, e = v3 * v3;
  for (int c = 0; c < 3; ++c) {
    const double x = (double)p[c * HW + q];
    const double pd = a * (double)v[c * HW + q] + x * v3;   // the tangent of rgb * a
    f[c] = s * a * pd;
    fa = fa + x * pd;
    e = e + pd * pd;
  }
  f[3] = s * fa;
  return e;
}

// grid (B): one workgroup per sample.  losses / dlosses come from the per-sample bodies and the per-cell
// gradients the other tap kernels use (dlosses: gnca_tap_loss_tangent's sum for one direction); every field
// value is rounded to fp32 once; quad is a fixed-order fp64 sum (per thread over its cells, then block_sum).
template <int KIND>
__global__ __launch_bounds__(kThreads) void gnca_tap_curvature(const TapCurvArgs a) {
  __shared__ double red[kThreads / 64];
  const int tid = threadIdx.x, b = blockIdx.x;
  const size_t HW = (size_t)a.m.H * a.m.W;
  const float* p = a.state + (size_t)b * a.sstride;
  const float* tg = a.tgt + (size_t)b * a.tbs;
  const float* vb = a.v + (size_t)b * a.vbs;
  float* fb = a.field + (size_t)b * a.fbs;
  int32_t cnt = 0;
  if (KIND == GNCA_TAP_PREMULT) {
    if (a.losses != nullptr) {   // (uniform over the workgroup)
      const float l = premult_loss_sample(a.m.H, a.m.W, p, tg, red);
      if (tid == 0) a.losses[b] = l;
    }
  } else {
    const float l = masked_loss_sample(a.m, p, tg, red, &cnt);   // (the count is the field's denominator)
    if (tid == 0) {
      if (a.losses != nullptr) a.losses[b] = l;
      if (a.alive_count != nullptr) a.alive_count[b] = cnt;
    }
  }
  if (a.dlosses != nullptr) {   // (uniform over the workgroup)
    double acc = 0.0;
    for (size_t q = tid; q < HW; q += kThreads) {
      float g[4];
      if (KIND == GNCA_TAP_PREMULT) premult_grad_cell(HW, p, tg, q, 1.f, g);
      else masked_grad_cell(a.m, HW, p, tg, q, 1.f, cnt, g);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc += (double)g[c] * (double)vb[c * HW + q];   // (the product is exact)
    }
    const double s = block_sum(acc, red);
    if (tid == 0) a.dlosses[b] = s;
  }
  double e = 0.0;
  if (KIND == GNCA_TAP_PREMULT) {
    const double s = 2.0 / (4.0 * (double)HW);
    for (size_t q = tid; q < HW; q += kThreads) {
      double f[4];
      e += premult_curv_cell(HW, p, vb, q, s, f);
#pragma unroll
      for (int c = 0; c < 4; ++c) fb[c * HW + q] = (float)f[c];
    }
    e = s * block_sum(e, red);
  } else {
    const double D = (double)cnt + 1e-8;   // (masked_grad_cell's denominator)
    for (size_t q = tid; q < HW; q += kThreads) {
      const bool alive = tg[3 * HW + q] > a.m.alpha_thr;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double x = (double)vb[c * HW + q];
        fb[c * HW + q] = alive ? (float)(2.0 * x / D) : 0.f;
        if (alive) e += x * x;
      }
    }
    e = 2.0 * block_sum(e, red) / D;
  }
  if (tid == 0) a.quad[b] = e;
}

// one rounded fp32 product, kept out of an FMA with the sum it feeds
__device__ __forceinline__ float mul_rn(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}

struct FieldInjectArgs {
  int B, C;
  size_t HW;
  const float* field;         // [B][4][H][W], contiguous
  float scale;
  float* dst;                 // [B,C,H,W]
};

// one thread per cell (b, q).  !FIRST: dst[b, c<4, q] += scale * field.  FIRST: every channel of dst is written,
// scale * field on channels 0..3 and zeros on the rest (gnca_tap_inject's FULL form without a source).
template <bool FIRST>
__global__ __launch_bounds__(kThreads) void gnca_field_inject(const FieldInjectArgs a) {
  const size_t HW = a.HW, total = (size_t)a.B * HW, ss = (size_t)a.C * HW;
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (size_t)gridDim.x * kThreads) {
    const size_t b = e / HW, q = e - b * HW;
    const float* f = a.field + b * 4 * HW + q;
    float* o = a.dst + b * ss + q;
    if (!FIRST) {
      for (int c = 0; c < 4; ++c) o[c * HW] = add_rn(o[c * HW], mul_rn(a.scale, f[c * HW]));
    } else {
      for (int c = 0; c < 4; ++c) o[c * HW] = mul_rn(a.scale, f[c * HW]);
      for (int c = 4; c < a.C; ++c) o[c * HW] = 0.f;
    }
  }
}

// the stability phase: per-sample fp64 sums of the close samples (the others are not read) ...
__global__ __launch_bounds__(kThreads) void gnca_stability_partial(int H, int W, const float* pred, long pbs,
                                                                   const float* tgt, long tbs, const uint8_t* close,
                                                                   double* part) {
  __shared__ double red[kThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (!close[b]) {   // (uniform over the workgroup)
    if (tid == 0) part[b] = 0.0;
    return;
  }
  const size_t n = 4 * (size_t)H * W;
  const float* p = pred + (size_t)b * pbs;
  const float* t = tgt + (size_t)b * tbs;
  double acc = 0.0;
  for (size_t e = tid; e < n; e += kThreads) {
    const double r = (double)(p[e] - t[e]);
    acc = fma(r, r, acc);
  }
  acc = block_sum(acc, red);
  if (tid == 0) part[b] = acc;
}

// ... then one workgroup adds them in a fixed order, counts the close samples and writes the scale
__global__ __launch_bounds__(kThreads) void gnca_stability_finish(int B, int H, int W, const uint8_t* close,
                                                                  const double* part, float* loss, float* scale) {
  __shared__ double red[kThreads / 64];
  double acc = 0.0, cnt = 0.0;
  for (int b = threadIdx.x; b < B; b += kThreads)
    if (close[b]) {
      acc += part[b];
      cnt += 1.0;
    }
  acc = block_sum(acc, red);
  cnt = block_sum(cnt, red);
  if (threadIdx.x == 0) {
    const double sc = cnt > 0.0 ? 1.0 / (cnt * 4.0 * (double)H * (double)W) : 0.0;
    loss[0] = (float)(acc * sc);
    scale[0] = (float)sc;
  }
}

__global__ __launch_bounds__(kThreads) void gnca_stability_bwd(int B, int H, int W, const float* pred, long pbs,
                                                               const float* tgt, long tbs, const uint8_t* close,
                                                               const float* scale, const float* g, float* gp,
                                                               long gbs) {
  const size_t n = 4 * (size_t)H * W, total = (size_t)B * n;
  const float s = 2.f * g[0] * scale[0];
  for (size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (size_t)gridDim.x * kThreads) {
    const size_t b = e / n, q = e - b * n;
    gp[b * gbs + q] = close[b] ? s * (pred[b * pbs + q] - tgt[b * tbs + q]) : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------
// Image metrics (train_graph_augmented_nca.py:405-422 and skimage's defaults): per image
// mse / pixel-perfect fraction / psnr / ssim of P = (pred_rgb * pred_alpha, pred_alpha) against the
// premultiplied target, for the whole batch in one launch.
//
// One workgroup per (image, band of kMetBand window rows).  The band's rows of X = clip(P_rgb) and
// Y = clip(T_rgb) are staged in LDS as fp32, in column chunks of kMetCols windows (+6 halo), so any
// H and W work.  While staging, each cell a band owns adds its squared errors and its pixel-perfect
// bit.  Then one thread per (colour channel, window column) walks down the band with running fp64
// window sums: the 7-tap horizontal sums of the entering row are added and those of the leaving row,
// kept in a register ring, subtracted (7 taps per moment and window instead of 49).  The tile
// geometry depends on (H, W) alone and every sum has a fixed order (per thread, xor-shuffle, waves,
// bands), so an image's result is bitwise the same whatever the batch around it.  The kernel is bound
// by fp64 VALU issue, not by traffic.
// ---------------------------------------------------------------------------------------------
constexpr int kMetWin = 7;                        // skimage's default win_size
constexpr int kMetBand = 22;                      // window rows per workgroup (72^2: 3 bands)
constexpr int kMetCols = 72;                      // window columns per chunk (52 KB LDS: 3 WGs per CU)
constexpr int kMetRin = kMetBand + kMetWin - 1;   // staged rows
constexpr int kMetCin = kMetCols + kMetWin - 1;   // staged columns
static_assert(3 * kMetCols <= kThreads, "one thread per (colour channel, window column)");

// the 7-tap sums of x, y, xx, yy, xy along one staged row, in fp64
__device__ __forceinline__ void met_hsum(const float* xr, const float* yr, double h[5]) {
  h[0] = h[1] = h[2] = h[3] = h[4] = 0.0;
#pragma unroll
  for (int k = 0; k < kMetWin; ++k) {
    const double x = (double)xr[k], y = (double)yr[k];
    h[0] += x; h[1] += y; h[2] += x * x; h[3] += y * y; h[4] += x * y;
  }
}

// skimage's S for one window (uniform filter, sample covariance, data_range 1) from its five raw
// sums a = Sx, b = Sy, Sxx, Syy, Sxy, with the 1/49 of the means and the 49/48 of the covariances
// moved into the constants: mx = a/49 and vx = (49 Sxx - a^2) / (48 * 49), so
//   S = (2ab + K1)(2 cxy + K2) / ((a^2 + b^2 + K1)(cxx + cyy + K2)),  cxy = 49 Sxy - ab, ...
// with K1 = 49^2 C1, K2 = 48 * 49 C2 (29 fp64 instructions instead of 40).
__device__ __forceinline__ double met_ssim_window(const double v[5]) {
#pragma clang fp contract(off)   // pred == target: numerator and denominator round alike, S == 1
  constexpr double n = (double)(kMetWin * kMetWin);
  constexpr double K1 = 1e-4 * n * n, K2 = 9e-4 * n * (n - 1.0);
  const double ab = v[0] * v[1], aa = v[0] * v[0], bb = v[1] * v[1];
  const double cxx = fma(n, v[2], -aa), cyy = fma(n, v[3], -bb), cxy = fma(n, v[4], -ab);
  const double num = fma(2.0, ab, K1) * fma(2.0, cxy, K2);
  const double den = ((aa + bb) + K1) * ((cxx + cyy) + K2);
  return num / den;
}

// sums {squared error over 4 channels, pixel-perfect cells, clipped squared error over rgb, S over
// windows and colour channels} -> out[0..3]
__device__ __forceinline__ void met_finish(const double s[4], int H, int W, float* out) {
  const double HW = (double)H * (double)W;
  out[0] = (float)(s[0] / (4.0 * HW));
  out[1] = (float)(s[1] / HW);
  out[2] = s[2] == 0.0 ? INFINITY : (float)(10.0 * log10(1.0 / (s[2] / (3.0 * HW))));
  out[3] = (H < kMetWin || W < kMetWin)
               ? NAN
               : (float)(s[3] / (3.0 * (double)(H - kMetWin + 1) * (double)(W - kMetWin + 1)));
}

__global__ __launch_bounds__(kThreads) void gnca_image_metrics(int nb, int H, int W, const float* pred, long pbs,
                                                               const float* tgt, long tbs, double* part,
                                                               float* out) {
  __shared__ float xs[3][kMetRin][kMetCin];
  __shared__ float ys[3][kMetRin][kMetCin];
  __shared__ double red[kThreads / 64][4];
  const int tid = threadIdx.x;
  const int n = blockIdx.x / nb, band = blockIdx.x - n * nb;
  const size_t HW = (size_t)H * W;
  const float* p = pred + (size_t)n * pbs;
  const float* t = tgt + (size_t)n * tbs;
  const int OH = H - (kMetWin - 1), OW = W - (kMetWin - 1);   // window rows / columns (<= 0: none)
  const int o0 = band * kMetBand;                             // first window row = first staged row
  const int nout = min(kMetBand, OH - o0);                    // window rows of this band (<= 0: none)
  const bool last_band = band == nb - 1;
  const int rin = min(kMetRin, H - o0);                       // staged rows
  const int own_r = last_band ? rin : kMetBand;               // rows whose cells this band counts
  const int ch = tid / kMetCols, col = tid - ch * kMetCols;
  double s_se4 = 0.0, s_pp = 0.0, s_se3 = 0.0, s_ss = 0.0;
  const int nchunk = (max(OW, 1) + kMetCols - 1) / kMetCols;
  for (int q = 0; q < nchunk; ++q) {
    const int c0 = q * kMetCols;
    const int cin = min(kMetCin, W - c0);                     // staged columns
    const int own_c = q == nchunk - 1 ? cin : kMetCols;       // columns whose cells this chunk counts
    const int cout = min(kMetCols, OW - c0);                  // window columns (<= 0: none)
    for (int e = tid; e < rin * kMetCin; e += kThreads) {
      const int r = e / kMetCin, c = e - r * kMetCin;
      if (c >= cin) continue;
      const size_t cell = (size_t)(o0 + r) * W + (size_t)(c0 + c);
      const float a = p[3 * HW + cell];
      const bool own = r < own_r && c < own_c;
      const float da = __fsub_rn(a, t[3 * HW + cell]);
      bool ok = fabsf(da) < 0.05f;
      double se4 = (double)a - (double)t[3 * HW + cell];
      se4 *= se4;
      double se3 = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float pv = __fmul_rn(p[k * HW + cell], a);      // the premultiply, rounded to fp32
        const float tv = t[k * HW + cell];
        ok = ok && fabsf(__fsub_rn(pv, tv)) < 0.05f;
        const double d = (double)pv - (double)tv;
        se4 += d * d;
        const float x = fminf(fmaxf(pv, 0.f), 1.f), y = fminf(fmaxf(tv, 0.f), 1.f);
        const double dc = (double)x - (double)y;
        se3 += dc * dc;
        xs[k][r][c] = x;
        ys[k][r][c] = y;
      }
      if (own) {
        s_se4 += se4;
        s_se3 += se3;
        s_pp += ok ? 1.0 : 0.0;
      }
    }
    __syncthreads();
    if (nout > 0 && ch < 3 && col < cout) {
      // ring[r % 7] keeps the horizontal sums of staged row r while it is inside the window: every
      // row's sums are computed once.  The row loop is unrolled by 7 so that the ring stays in registers.
      double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, ring[kMetWin][5];
#pragma unroll
      for (int r = 0; r < kMetWin - 1; ++r) {
        met_hsum(&xs[ch][r][col], &ys[ch][r][col], ring[r]);
#pragma unroll
        for (int m = 0; m < 5; ++m) v[m] += ring[r][m];
      }
      for (int ob = 0; ob < nout; ob += kMetWin) {
#pragma unroll
        for (int k = 0; k < kMetWin; ++k) {
          const int o = ob + k;                       // window rows o .. o + 6; o % 7 == k
          if (o < nout) {
            constexpr int kw = kMetWin;
            const int in = (k + kw - 1) % kw;         // the slot of the entering row o + 6
            met_hsum(&xs[ch][o + kw - 1][col], &ys[ch][o + kw - 1][col], ring[in]);
#pragma unroll
            for (int m = 0; m < 5; ++m) v[m] += ring[in][m];
            s_ss += met_ssim_window(v);
#pragma unroll
            for (int m = 0; m < 5; ++m) v[m] -= ring[k][m];   // the leaving row o
          }
        }
      }
    }
    __syncthreads();
  }
  double s[4] = {s_se4, s_pp, s_se3, s_ss};
#pragma unroll
  for (int m = 0; m < 4; ++m)
    for (int off = 32; off > 0; off >>= 1) s[m] += __shfl_xor(s[m], off);
  if ((tid & 63) == 0)
    for (int m = 0; m < 4; ++m) red[tid >> 6][m] = s[m];
  __syncthreads();
  if (tid == 0) {
    for (int m = 0; m < 4; ++m) {
      double v = 0.0;
      for (int w = 0; w < kThreads / 64; ++w) v += red[w][m];
      s[m] = v;
    }
    if (nb == 1) {
      met_finish(s, H, W, out + (size_t)n * 4);
    } else {
      for (int m = 0; m < 4; ++m) part[((size_t)n * nb + band) * 4 + m] = s[m];
    }
  }
}

// the bands' partial sums of each image, added in band order
__global__ __launch_bounds__(kThreads) void gnca_image_metrics_finish(int N, int nb, int H, int W,
                                                                      const double* part, float* out) {
  const int n = blockIdx.x * kThreads + threadIdx.x;
  if (n >= N) return;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < nb; ++b)
    for (int m = 0; m < 4; ++m) s[m] += part[((size_t)n * nb + b) * 4 + m];
  met_finish(s, H, W, out + (size_t)n * 4);
}

// bands per image: a function of H alone (0: too many workgroups for one launch)
int met_bands(int32_t N, int32_t H) {
  const int OH = H - (kMetWin - 1);
  const long nb = ((OH > 1 ? OH : 1) + kMetBand - 1) / kMetBand;
  return nb * (long)N > 0x7fffffffL ? 0 : (int)nb;
}

// ---------------------------------------------------------------------------------------------
// State vitals (include/gnca.h, gnca_state_vitals): how much of a state is alive, where its pattern
// lies and whether it is still finite, for the whole batch in one pass over the state.
//
// One workgroup per (sample, band of kVitBand rows, chunk of kVitCols columns).  The tile's alpha
// cells and a one-cell halo around them are staged in LDS (cells outside the image as -inf: they
// never pass a threshold), so the 3x3 pool, the counts, the sums, the centroid and the bounding box
// come from LDS; the other C - 1 planes are read once each with kVitU loads per thread in flight
// (V = 4 where W % 4 == 0: four cells per thread, one 16-byte load where the addresses allow it, else
// four 4-byte loads of the same cells, so the order of every sum depends on the shape alone) and feed
// max_abs, nonfinite and the hidden sum of squares.  Every sum is fp64 (counts as fp64 integers) in an order fixed by (C, H, W): per thread, xor-shuffle, the
// waves in order, then the tiles' partials by one wave per sample (lane l adds tiles l, l + 64, ...,
// then the same butterfly).  A sample's 13 numbers are therefore bitwise the same in any batch.
// ---------------------------------------------------------------------------------------------
constexpr int kVitBand = GNCA_VITALS_BAND_ROWS;   // rows per workgroup
constexpr int kVitCols = GNCA_VITALS_TILE_COLS;   // columns per workgroup (10 KB LDS)
static_assert(kVitCols % 4 == 0, "a tile starts on a 16-byte column where W % 4 == 0");
constexpr int kVitU = 5;                          // planes a thread has in flight
constexpr int kVitF = GNCA_VITALS_FIELDS;
constexpr double kVitNoCell = 2147483647.0;       // y0 / x0 of a tile without a mature cell

// Partials, one kVitF-vector per tile: the output fields' order, with Σ clip·i and Σ clip·j in place
// of the centroid and Σ v² in place of the rms.  Fields 6 and 8 combine by min, 7, 9 and 10 by max,
// the others by addition.
__device__ __forceinline__ double vit_combine(int f, double a, double b) {
  if (f == 6 || f == 8) return fmin(a, b);
  if (f == 7 || f == 9 || f == 10) return fmax(a, b);
  return a + b;
}

__device__ __forceinline__ double vit_identity(int f) {
  if (f == 6 || f == 8) return kVitNoCell;
  if (f == 7 || f == 9) return -1.0;
  return 0.0;
}

// every lane of the wave calls it: all lanes end with the wave's combined partials
__device__ __forceinline__ void vit_wave_reduce(double s[kVitF]) {
#pragma unroll
  for (int f = 0; f < kVitF; ++f)
    for (int off = 32; off > 0; off >>= 1) s[f] = vit_combine(f, s[f], __shfl_xor(s[f], off));
}

// one value of any plane: the largest finite magnitude, the non-finite count and (hidden planes)
// the finite values' sum of squares
__device__ __forceinline__ void vit_value(float v, bool hidden, float& mx, int& nf, double& hs) {
  const float av = fabsf(v);
  const bool fin = av <= 3.402823466e+38f;   // false for NaN and +-inf
  mx = fmaxf(mx, fin ? av : 0.f);
  nf += fin ? 0 : 1;
  if (hidden) {   // (uniform over the workgroup)
    const double d = fin ? (double)v : 0.0;
    hs = fma(d, d, hs);
  }
}

template <int V, bool A>
__global__ __launch_bounds__(kThreads) void gnca_state_vitals_k(int C, int H, int W, int nbands, int nchunks,
                                                                const float* x, long xbs, float thr,
                                                                double* part) {
  typedef float vf __attribute__((ext_vector_type(V)));
  __shared__ float as[kVitBand + 2][kVitCols + 2];
  __shared__ double red[kThreads / 64][kVitF];
  const int tid = threadIdx.x;
  const int chunk = (int)(blockIdx.x % (unsigned)nchunks);
  const int sb = (int)(blockIdx.x / (unsigned)nchunks);
  const int band = sb % nbands, b = sb / nbands;
  const size_t HW = (size_t)H * W;
  const float* xb = x + (size_t)b * xbs;
  const int r0 = band * kVitBand, nr = min(kVitBand, H - r0);   // 1 .. kVitBand rows
  const int c0 = chunk * kVitCols, nc = min(kVitCols, W - c0);  // 1 .. kVitCols columns
  float mx = 0.f;
  int nf = 0;
  double hs = 0.0;

  // the alpha tile and its halo: as[tr][tc] = alpha(r0 - 1 + tr, c0 - 1 + tc)
  const float* ap = xb + 3 * HW;
  const int tw = nc + 2;
  for (int e = tid; e < (nr + 2) * tw; e += kThreads) {
    const int tr = e / tw, tc = e - tr * tw;
    const int i = r0 - 1 + tr, j = c0 - 1 + tc;
    float a = -INFINITY;
    if (i >= 0 && i < H && j >= 0 && j < W) {
      a = ap[(size_t)i * W + j];
      if (tr >= 1 && tr <= nr && tc >= 1 && tc <= nc) vit_value(a, false, mx, nf, hs);   // the tile's own cells
    }
    as[tr][tc] = a;
  }

  // the other planes: q = 0..2 are the colours, q >= 3 the hidden channels q + 1
  const int nvc = nc / V;   // (V = 4 only where W % 4 == 0, and kVitCols % 4 == 0)
  for (int e = tid; e < nr * nvc; e += kThreads) {
    const int r = e / nvc, v = e - r * nvc;
    const float* p = xb + (size_t)(r0 + r) * W + (size_t)(c0 + V * v);
    for (int q0 = 0; q0 < C - 1; q0 += kVitU) {
      vf val[kVitU];
#pragma unroll
      for (int u = 0; u < kVitU; ++u) {
        const int q = q0 + u;
        if (q < C - 1) {
          const float* pq = p + (size_t)(q < 3 ? q : q + 1) * HW;
          if constexpr (A) {
            val[u] = *reinterpret_cast<const vf*>(pq);
          } else {
#pragma unroll
            for (int l = 0; l < V; ++l) val[u][l] = pq[l];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kVitU; ++u) {
        const int q = q0 + u;
        if (q < C - 1) {
#pragma unroll
          for (int l = 0; l < V; ++l) vit_value(val[u][l], q >= 3, mx, nf, hs);
        }
      }
    }
  }
  __syncthreads();

  int alive = 0, mature = 0, y0 = 0x7fffffff, y1 = -1, x0 = 0x7fffffff, x1 = -1;
  double asum = 0.0, mass = 0.0, sy = 0.0, sx = 0.0;
  for (int e = tid; e < nr * nc; e += kThreads) {
    const int r = e / nc, c = e - r * nc;
    float m = -INFINITY;   // the 3x3 pool around as[r + 1][c + 1]
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, as[r + dy][c + dx]);
    const float a = as[r + 1][c + 1];
    const int i = r0 + r, j = c0 + c;
    alive += m > thr ? 1 : 0;
    if (a > thr) {
      ++mature;
      y0 = min(y0, i); y1 = max(y1, i); x0 = min(x0, j); x1 = max(x1, j);
    }
    const double cl = (double)fminf(fmaxf(a, 0.f), 1.f);
    asum += (double)a;
    mass += cl;
    sy = fma(cl, (double)i, sy);   // (the products are exact)
    sx = fma(cl, (double)j, sx);
  }

  double s[kVitF] = {(double)alive, (double)mature, asum, mass, sy, sx, (double)y0, (double)y1,
                     (double)x0,    (double)x1,     (double)mx, (double)nf, hs};
  vit_wave_reduce(s);
  if ((tid & 63) == 0)
#pragma unroll
    for (int f = 0; f < kVitF; ++f) red[tid >> 6][f] = s[f];
  __syncthreads();
  if (tid < kVitF) {
    double v = red[0][tid];
    for (int w = 1; w < kThreads / 64; ++w) v = vit_combine(tid, v, red[w][tid]);
    part[(size_t)blockIdx.x * kVitF + tid] = v;
  }
}

// one wave per sample: its tiles' partials combined in a fixed order, then the 13 fields
__global__ __launch_bounds__(kThreads) void gnca_state_vitals_finish(int B, int C, int H, int W, int np,
                                                                     const double* part, double* out) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (b >= B) return;   // (uniform over the wave)
  double s[kVitF];
#pragma unroll
  for (int f = 0; f < kVitF; ++f) s[f] = vit_identity(f);
  for (int p = lane; p < np; p += 64) {
    const double* q = part + ((size_t)b * np + p) * kVitF;
#pragma unroll
    for (int f = 0; f < kVitF; ++f) s[f] = vit_combine(f, s[f], q[f]);
  }
  vit_wave_reduce(s);
  if (lane != 0) return;
  double* o = out + (size_t)b * kVitF;
  const bool none = s[1] == 0.0;
  o[0] = s[0];
  o[1] = s[1];
  o[2] = s[2];
  o[3] = s[3];
  o[4] = s[4] / s[3];   // (0 / 0: NaN)
  o[5] = s[5] / s[3];
#pragma unroll
  for (int f = 6; f < 10; ++f) o[f] = none ? -1.0 : s[f];
  o[10] = s[10];
  o[11] = s[11];
  o[12] = C > 4 ? sqrt(s[12] / ((double)(C - 4) * (double)H * (double)W)) : 0.0;
}

// tiles per sample: a function of (H, W) alone (0: too many workgroups for one launch)
long vit_tiles(int32_t B, int32_t H, int32_t W, int* nbands, int* nchunks) {
  *nbands = (H + kVitBand - 1) / kVitBand;
  *nchunks = (W + kVitCols - 1) / kVitCols;
  const long np = (long)*nbands * *nchunks;
  return np * (long)B > 0x7fffffffL ? 0 : np;
}

// ---------------------------------------------------------------------------------------------
// The iteration's tail (train_graph_augmented_nca.py:367-391, train_intermediate_loss.py:269-296):
// gradient policy + Adam over a by-value table of tensors, and the pool write-back.  Both move a few
// tens of KB: what counts is one launch, no host wait and a fixed summation order.
// ---------------------------------------------------------------------------------------------
constexpr int kOptChunk = 2048;      // elements per update workgroup: two float4 per thread
constexpr int kCommitChunk = 4096;   // floats per copy workgroup: four float4 per thread

// the sum of squares of g[0 .. n), in every thread: thread t adds the quads t, t + kThreads, ...
// element by element, then element 4 (n / 4) + t of the tail, then block_sum.  The order depends on
// n alone: a 16-byte-aligned g is read with float4 loads, any other with scalar loads of the same
// elements in the same order (the squares are exact in fp64, so the bits agree).
__device__ inline double tensor_sumsq(const float* g, int64_t n, double* red) {
  const int tid = threadIdx.x;
  const int64_t nq = n >> 2;
  double acc = 0.0;
  if (((uintptr_t)g & 15) == 0) {
    for (int64_t q = tid; q < nq; q += kThreads) {
      const f4 x = *reinterpret_cast<const f4*>(g + 4 * q);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += (double)x[k] * (double)x[k];
    }
  } else {
    for (int64_t q = tid; q < nq; q += kThreads)
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += (double)g[4 * q + k] * (double)g[4 * q + k];
  }
  if (tid < (int)(n & 3)) acc += (double)g[4 * nq + tid] * (double)g[4 * nq + tid];
  return block_sum(acc, red);
}

__global__ __launch_bounds__(kThreads) void gnca_optim_sumsq(const gnca_optim_desc d) {
  __shared__ double red[kThreads / 64];
  const int i = blockIdx.x;
  const double s = tensor_sumsq(d.t[i].g, d.t[i].numel, red);
  if (threadIdx.x == 0) d.sumsq[d.sumsq_base + i] = s;
}

// torch's Adam, one element (torch/optim/adam.py:_single_tensor_adam and the pointwise kernels it
// calls: add(alpha), lerp, mul + addcmul, sqrt / bias + eps, addcdiv), after the gradient policy
struct OptimConsts {
  bool normalize;   // g / div (the tensor's norm + norm_eps)
  float div, mul;   // mul: the clip coefficient (1 for the other policies)
  float wd, w1, b2, w2, bc2s, eps, nstep;
};

__device__ __forceinline__ void adam_element(const OptimConsts& k, float g, float& p, float& m, float& v) {
  if (k.normalize) g = g / k.div;
  g = g * k.mul;
  if (k.wd != 0.f) g = g + k.wd * p;
  const float diff = g - m;
  m = k.w1 < 0.5f ? m + k.w1 * diff : g - diff * (1.f - k.w1);
  v = v * k.b2 + (k.w2 * g) * g;
  const float den = sqrtf(v) / k.bc2s + k.eps;
  p = p + (k.nstep * m) / den;
}

// one workgroup per kOptChunk elements of one tensor
__global__ __launch_bounds__(kThreads) void gnca_optim_update(const gnca_optim_desc d) {
  __shared__ double red[kThreads / 64];
  int i = 0;
  int64_t c = blockIdx.x;
  for (; i < d.num_tensors; ++i) {   // (uniform over the workgroup)
    const int64_t nc = (d.t[i].numel + kOptChunk - 1) / kOptChunk;
    if (c < nc) break;
    c -= nc;
  }
  if (i >= d.num_tensors) return;
  const gnca_optim_tensor t = d.t[i];
  OptimConsts k;
  k.normalize = d.policy == GNCA_OPTIM_POLICY_NORMALIZE;
  k.div = 1.f;
  k.mul = 1.f;
  if (k.normalize) {
    const double ss = d.sumsq ? d.sumsq[d.sumsq_base + i] : tensor_sumsq(t.g, t.numel, red);
    k.div = (float)sqrt(ss) + (float)d.norm_eps;
  } else if (d.policy == GNCA_OPTIM_POLICY_CLIP) {
    double tot = 0.0;
    if (d.sumsq) {
      for (int j = 0; j < d.sumsq_count; ++j) tot += d.sumsq[j];
    } else {
      for (int j = 0; j < d.num_tensors; ++j) tot += tensor_sumsq(d.t[j].g, d.t[j].numel, red);
    }
    const float coef = (float)d.max_norm / ((float)sqrt(tot) + 1e-6f);
    k.mul = coef > 1.f ? 1.f : coef;   // (a NaN norm stays NaN, as torch.clamp leaves it)
  }
  k.wd = (float)t.weight_decay;
  k.w1 = (float)(1.0 - d.beta1);
  k.b2 = (float)d.beta2;
  k.w2 = (float)(1.0 - d.beta2);
  k.bc2s = (float)sqrt(t.bias2);
  k.eps = (float)d.eps;
  k.nstep = (float)(-(t.lr / t.bias1));
  const int tid = threadIdx.x;
  const int64_t e0 = c * kOptChunk;
  const int64_t n = t.numel - e0 < kOptChunk ? t.numel - e0 : kOptChunk;   // this chunk's elements
  float* p = t.p + e0;
  const float* g = t.g + e0;
  float* m = t.m + e0;
  float* v = t.v + e0;
  const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  const int64_t nv = vec ? (n & ~(int64_t)3) : 0;   // elements done with 16-byte accesses
  for (int64_t e = 4 * (int64_t)tid; e < nv; e += 4 * kThreads) {
    const f4 gv = *reinterpret_cast<const f4*>(g + e);
    f4 pv = *reinterpret_cast<f4*>(p + e), mv = *reinterpret_cast<f4*>(m + e), vv = *reinterpret_cast<f4*>(v + e);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float pe = pv[q], me = mv[q], ve = vv[q];
      adam_element(k, gv[q], pe, me, ve);
      pv[q] = pe; mv[q] = me; vv[q] = ve;
    }
    *reinterpret_cast<f4*>(p + e) = pv;
    *reinterpret_cast<f4*>(m + e) = mv;
    *reinterpret_cast<f4*>(v + e) = vv;
  }
  for (int64_t e = nv + tid; e < n; e += kThreads) adam_element(k, g[e], p[e], m[e], v[e]);
}

// The forward gradient.  Neither kernel lets a product join the sum that follows it
// in an FMA: every fp64 product and sum is rounded on its own, so the result is that of the plain formula.
// coef[k], one workgroup per k: the samples of tap r per thread (b = tid, tid + kThreads, ...), block_sum, then
// the taps in order.
__global__ __launch_bounds__(kThreads) void gnca_fgrad_coef(const gnca_forward_grad_desc d) {
#pragma clang fp contract(off)
  __shared__ double red[kThreads / 64];
  const int k = blockIdx.x;
  double acc = 0.0;
  for (int r = 0; r < d.R; ++r) {
    const double* row = d.dlosses + ((size_t)r * d.K + k) * d.B;
    double s = 0.0;
    for (int b = threadIdx.x; b < d.B; b += kThreads) s += row[b];
    s = block_sum(s, red);
    const double w = d.tap_weight ? (double)d.tap_weight[r] : 1.0;
    acc = acc + w * s;
  }
  if (threadIdx.x == 0) d.coef[k] = d.scale * acc;
}

// g of kOptChunk elements of one tensor per workgroup, one element per thread and pass (coalesced along the
// direction rows, whose alignment is arbitrary)
__global__ __launch_bounds__(kThreads) void gnca_fgrad_apply(const gnca_forward_grad_desc d) {
#pragma clang fp contract(off)
  int i = 0;
  int64_t c = blockIdx.x;
  for (; i < d.num_tensors; ++i) {   // (uniform over the workgroup)
    const int64_t nc = (d.t[i].numel + kOptChunk - 1) / kOptChunk;
    if (c < nc) break;
    c -= nc;
  }
  if (i >= d.num_tensors) return;
  const gnca_forward_grad_tensor t = d.t[i];
  const int64_t e0 = c * kOptChunk;
  const int64_t e1 = t.numel - e0 < kOptChunk ? t.numel : e0 + kOptChunk;
  const bool accumulate = (d.flags & GNCA_FGRAD_ACCUMULATE) != 0;
  for (int64_t e = e0 + threadIdx.x; e < e1; e += kThreads) {
    double s = 0.0;
    for (int k = 0; k < d.K; ++k) {
      const double term = d.coef[k] * (double)t.dir[(int64_t)k * t.dir_stride + e];
      s = s + term;
    }
    const float v = (float)s;
    t.g[e] = accumulate ? t.g[e] + v : v;
  }
}

// does loss `o` of sample j rank before loss `mine` of sample b (torch.topk's descending order, a
// NaN above every number; ties and NaNs among themselves by lower index)?
__device__ __forceinline__ bool ranks_before(float o, int j, float mine, int b) {
  const bool on = o != o, mn = mine != mine;
  if (on != mn) return on;
  if (on || o == mine) return j < b;
  return o > mine;
}

// one workgroup per (sample, kCommitChunk floats): each ranks its own sample, picks its source and
// copies its chunk into the sample's slot
__global__ __launch_bounds__(kThreads) void gnca_pool_commit_copy(const gnca_pool_commit_desc d, int chunks,
                                                                  float* pool, const int64_t* slots,
                                                                  const float* state, const float* per,
                                                                  const float* seeds, const float* seed1,
                                                                  const int64_t* rand_idx) {
  __shared__ int cnt[kThreads / 64];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / chunks, c = blockIdx.x - b * chunks;
  const int64_t E = d.sample_elems;
  const int64_t slot = slots[b];
  if (slot < 0 || slot >= d.pool_slots) return;   // (uniform over the workgroup)
  const float* src = state + (int64_t)b * E;
  if (rand_idx != nullptr && *rand_idx == (int64_t)b) {
    src = seed1;
  } else if (d.n_reset > 0) {
    const float mine = per[b];
    int r = 0;
    for (int j = tid; j < d.B; j += kThreads) r += ranks_before(per[j], j, mine, b) ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) r += __shfl_xor(r, off);
    if ((tid & 63) == 0) cnt[tid >> 6] = r;
    __syncthreads();
    r = 0;
    for (int w = 0; w < kThreads / 64; ++w) r += cnt[w];
    if (r < d.n_reset) src = seeds + (int64_t)r * E;
  }
  const int64_t e0 = (int64_t)c * kCommitChunk;
  const int64_t n = E - e0 < kCommitChunk ? E - e0 : kCommitChunk;
  src += e0;
  float* dst = pool + slot * E + e0;
  const bool vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
  const int64_t nv = vec ? (n & ~(int64_t)3) : 0;
  for (int64_t e = 4 * (int64_t)tid; e < nv; e += 4 * kThreads)
    *reinterpret_cast<f4*>(dst + e) = *reinterpret_cast<const f4*>(src + e);
  for (int64_t e = nv + tid; e < n; e += kThreads) dst[e] = src[e];
}

}  // namespace
}  // namespace gnca

using namespace gnca;

extern "C" int gnca_optim_step(const gnca_optim_desc* d, void* stream) {
  if (!d || d->num_tensors < 0 || d->num_tensors > GNCA_OPTIM_MAX_TENSORS) return GNCA_ERR_INVALID;
  if (d->policy < GNCA_OPTIM_POLICY_NONE || d->policy > GNCA_OPTIM_POLICY_CLIP) return GNCA_ERR_INVALID;
  if (d->flags & ~(GNCA_OPTIM_SUMSQ | GNCA_OPTIM_UPDATE)) return GNCA_ERR_INVALID;
  int64_t chunks = 0, elems = 0;
  for (int i = 0; i < d->num_tensors; ++i) {
    const gnca_optim_tensor& t = d->t[i];
    if (!t.p || !t.g || !t.m || !t.v || t.numel < 0) return GNCA_ERR_INVALID;
    chunks += (t.numel + kOptChunk - 1) / kOptChunk;
    elems += t.numel;
    if (chunks > 0x7fffffffLL) return GNCA_ERR_INVALID;
  }
  const bool sums = d->policy != GNCA_OPTIM_POLICY_NONE;
  if (sums && d->sumsq) {
    if (((uintptr_t)d->sumsq & 7) || d->sumsq_base < 0 || d->sumsq_count < 0 ||
        (int64_t)d->sumsq_base + d->num_tensors > (int64_t)d->sumsq_count)
      return GNCA_ERR_WORKSPACE;
  } else if (sums) {
    if (d->flags != 0) return GNCA_ERR_INVALID;
    if (elems > GNCA_OPTIM_ONE_LAUNCH_MAX) return GNCA_ERR_WORKSPACE;
  }
  if (d->num_tensors == 0) return GNCA_OK;
  const uint32_t flags = (sums && d->sumsq && d->flags) ? d->flags : (GNCA_OPTIM_SUMSQ | GNCA_OPTIM_UPDATE);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipSuccess;
  if (sums && d->sumsq && (flags & GNCA_OPTIM_SUMSQ)) {
    hipLaunchKernelGGL(gnca_optim_sumsq, dim3((unsigned)d->num_tensors), dim3(kThreads), 0, st, *d);
    e = hipGetLastError();
  }
  if (e == hipSuccess && (flags & GNCA_OPTIM_UPDATE) && chunks > 0) {
    hipLaunchKernelGGL(gnca_optim_update, dim3((unsigned)chunks), dim3(kThreads), 0, st, *d);
    e = hipGetLastError();
  }
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

extern "C" int gnca_pool_commit(const gnca_pool_commit_desc* d, float* pool, const int64_t* slots,
                                const float* state, const float* per_sample, const float* seeds,
                                const float* seed1, const int64_t* rand_idx, void* stream) {
  if (!d || d->B <= 0 || d->sample_elems <= 0 || d->pool_slots <= 0 || d->n_reset < 0 || d->n_reset > d->B)
    return GNCA_ERR_INVALID;
  if (!pool || !slots || !state) return GNCA_ERR_INVALID;
  if (d->n_reset > 0 && (!per_sample || !seeds)) return GNCA_ERR_INVALID;
  if ((rand_idx != nullptr) != (seed1 != nullptr)) return GNCA_ERR_INVALID;
  const int64_t chunks = (d->sample_elems + kCommitChunk - 1) / kCommitChunk;
  if (chunks * d->B > 0x7fffffffLL) return GNCA_ERR_INVALID;
  hipLaunchKernelGGL(gnca_pool_commit_copy, dim3((unsigned)(chunks * d->B)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), *d, (int)chunks, pool, slots, state, per_sample, seeds,
                     seed1, rand_idx);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

extern "C" int gnca_loss_premult_f32(int32_t B, int32_t H, int32_t W, const float* pred, int64_t pbs,
                                     const float* target, int64_t tbs, float* per_sample, void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || !pred || !target || !per_sample) return GNCA_ERR_INVALID;
  hipLaunchKernelGGL(gnca_loss_fwd, dim3(B), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), H, W,
                     pred, (long)pbs, target, (long)tbs, per_sample);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

extern "C" int gnca_loss_premult_bwd_f32(int32_t B, int32_t H, int32_t W, const float* pred, int64_t pbs,
                                         const float* target, int64_t tbs, const float* g, float* grad_pred,
                                         int64_t gbs, void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || !pred || !target || !g || !grad_pred) return GNCA_ERR_INVALID;
  const size_t total = (size_t)B * H * W;
  size_t blocks = (total + kThreads - 1) / kThreads;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(gnca_loss_bwd, dim3((unsigned)blocks), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream),
                     B, H, W, pred, (long)pbs, target, (long)tbs, g, grad_pred, (long)gbs);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

static bool masked_desc_ok(const gnca_masked_loss_desc* d) { return d && d->B > 0 && d->H > 0 && d->W > 0; }

// an elementwise launch's grid: one thread per element, grid-stride beyond 8192 workgroups
static unsigned elementwise_blocks(size_t total) {
  const size_t blocks = (total + kThreads - 1) / kThreads;
  return (unsigned)(blocks > 8192 ? 8192 : blocks);
}

extern "C" int gnca_loss_masked_f32(const gnca_masked_loss_desc* d, const float* pred, int64_t pbs,
                                    const float* target, int64_t tbs, float* per_sample, int32_t* alive_count,
                                    int32_t* nsteps_out, void* stream) {
  if (!masked_desc_ok(d) || !pred || !target || !per_sample || !alive_count || pbs < 0 || tbs < 0)
    return GNCA_ERR_INVALID;
  if (nsteps_out && d->close_steps < 0) return GNCA_ERR_INVALID;
  hipLaunchKernelGGL(gnca_masked_loss_fwd, dim3(d->B), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), *d,
                     pred, (long)pbs, target, (long)tbs, per_sample, alive_count, nsteps_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

extern "C" int gnca_loss_masked_bwd_f32(const gnca_masked_loss_desc* d, const float* pred, int64_t pbs,
                                        const float* target, int64_t tbs, const int32_t* alive_count,
                                        const float* g, float* grad_pred, int64_t gbs, void* stream) {
  if (!masked_desc_ok(d) || !pred || !target || !alive_count || !g || !grad_pred || pbs < 0 || tbs < 0 || gbs < 0)
    return GNCA_ERR_INVALID;
  hipLaunchKernelGGL(gnca_masked_loss_bwd, dim3(elementwise_blocks((size_t)d->B * d->H * d->W)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), *d, pred, (long)pbs, target, (long)tbs, alive_count, g,
                     grad_pred, (long)gbs);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

namespace gnca {

bool taps_ok(const gnca_step_desc* d, const gnca_rollout_sched* s, const gnca_rollout_taps* taps) {
  if (!d || !s || !taps || !taps->steps || !taps->target || taps->n < 1 || taps->target_bstride < 0) return false;
  if (d->B <= 0 || d->C < 4 || d->H <= 0 || d->W <= 0) return false;
  if (taps->kind != GNCA_TAP_PREMULT && taps->kind != GNCA_TAP_MASKED) return false;
  if (taps->masked.B != d->B || taps->masked.H != d->H || taps->masked.W != d->W) return false;   // (either kind)
  int prev = 0;
  for (int r = 0; r < taps->n; ++r) {
    const int t = taps->steps[r];
    if (t <= prev || t > s->steps) return false;
    prev = t;
  }
  return true;
}

int launch_tap_inject(const gnca_step_desc* d, const gnca_rollout_taps* taps, const float* state, const float* gl,
                      const int32_t* alive_count, const float* src, float* dst, bool full, hipStream_t st) {
  TapInjectArgs a;
  a.m = taps->masked;   // (B, H, W are the desc's: taps_ok)
  a.C = d->C;
  a.state = state; a.tgt = taps->target; a.tbs = (long)taps->target_bstride;
  a.alive_count = alive_count; a.gl = gl; a.src = src; a.dst = dst;
  const dim3 grid(elementwise_blocks((size_t)d->B * d->H * d->W)), block(kThreads);
  const bool masked = taps->kind == GNCA_TAP_MASKED;
  if (masked && full) hipLaunchKernelGGL((gnca_tap_inject<GNCA_TAP_MASKED, true>), grid, block, 0, st, a);
  else if (masked) hipLaunchKernelGGL((gnca_tap_inject<GNCA_TAP_MASKED, false>), grid, block, 0, st, a);
  else if (full) hipLaunchKernelGGL((gnca_tap_inject<GNCA_TAP_PREMULT, true>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((gnca_tap_inject<GNCA_TAP_PREMULT, false>), grid, block, 0, st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

// gnca_tap_loss for ONE tap whose state is given by address: a chunk of one tap whose step is the
// launch's own "T", so the kernel takes the x_final pointer, here `state`, and no tape is read
int launch_tap_loss_state(const gnca_step_desc* d, const gnca_rollout_taps* taps, int r, const float* state,
                          float* losses, int32_t* alive_count, hipStream_t st) {
  TapLossArgs a;
  a.m = taps->masked;   // (B, H, W are the desc's: taps_ok)
  a.T = taps->steps[r];
  a.tape = nullptr;
  a.slot = 0;
  a.sstride = (size_t)d->C * d->H * d->W;
  a.x_final = state;
  a.tgt = taps->target; a.tbs = (long)taps->target_bstride;
  a.losses = losses; a.alive_count = alive_count;
  TapChunk ch;
  ch.first = r;
  for (int j = 0; j < GNCA_TAP_CHUNK; ++j) ch.step[j] = j == 0 ? a.T : 0;
  const dim3 grid((unsigned)d->B, 1u), block(kThreads);
  if (taps->kind == GNCA_TAP_MASKED) hipLaunchKernelGGL(gnca_tap_loss<GNCA_TAP_MASKED>, grid, block, 0, st, a, ch);
  else hipLaunchKernelGGL(gnca_tap_loss<GNCA_TAP_PREMULT>, grid, block, 0, st, a, ch);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

// gnca_tap_loss_tangent on one state and its K tangents (m: validated by the caller; K >= 1)
int launch_tap_loss_tangent(int kind, const gnca_masked_loss_desc* m, int K, const float* state, size_t sstride,
                            const float* v, size_t vds, size_t vbs, const float* tgt, long tbs, float* losses,
                            double* dlosses, int32_t* alive_count, hipStream_t st) {
  TapLossTanArgs a;
  a.m = *m;
  a.K = K;
  a.state = state; a.sstride = sstride;
  a.tgt = tgt; a.tbs = tbs;
  a.v = v; a.vds = vds; a.vbs = vbs;
  a.losses = losses; a.dlosses = dlosses; a.alive_count = alive_count;
  const dim3 grid((unsigned)m->B, (unsigned)((K + kLossTanDirs - 1) / kLossTanDirs)), block(kThreads);
  if (kind == GNCA_TAP_MASKED) hipLaunchKernelGGL(gnca_tap_loss_tangent<GNCA_TAP_MASKED>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(gnca_tap_loss_tangent<GNCA_TAP_PREMULT>, grid, block, 0, st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

// gnca_tap_curvature on one state and one tangent of it (m: validated by the caller)
int launch_tap_curvature(int kind, const gnca_masked_loss_desc* m, const float* state, size_t sstride, const float* v,
                         size_t vbs, const float* tgt, long tbs, float* losses, double* dlosses, double* quad,
                         float* field, size_t fbs, int32_t* alive_count, hipStream_t st) {
  TapCurvArgs a;
  a.m = *m;
  a.state = state; a.sstride = sstride;
  a.tgt = tgt; a.tbs = tbs;
  a.v = v; a.vbs = vbs;
  a.losses = losses; a.dlosses = dlosses; a.quad = quad;
  a.field = field; a.fbs = fbs;
  a.alive_count = alive_count;
  const dim3 grid((unsigned)m->B), block(kThreads);
  if (kind == GNCA_TAP_MASKED) hipLaunchKernelGGL(gnca_tap_curvature<GNCA_TAP_MASKED>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(gnca_tap_curvature<GNCA_TAP_PREMULT>, grid, block, 0, st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

int launch_field_inject(const gnca_step_desc* d, const float* field, float scale, float* dst, bool first,
                        hipStream_t st) {
  FieldInjectArgs a;
  a.B = d->B; a.C = d->C;
  a.HW = (size_t)d->H * d->W;
  a.field = field; a.scale = scale; a.dst = dst;
  const dim3 grid(elementwise_blocks((size_t)d->B * a.HW)), block(kThreads);
  if (first) hipLaunchKernelGGL(gnca_field_inject<true>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(gnca_field_inject<false>, grid, block, 0, st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

}  // namespace gnca

extern "C" int gnca_loss_curvature(int32_t kind, const gnca_masked_loss_desc* d, const float* pred, int64_t pbs,
                                   const float* v, int64_t vbs, const float* target, int64_t tbs, float* losses,
                                   double* dlosses, double* quad, float* field, int64_t fbs, void* hip_stream) {
  if (kind != GNCA_TAP_PREMULT && kind != GNCA_TAP_MASKED) return GNCA_ERR_INVALID;
  if (!masked_desc_ok(d)) return GNCA_ERR_INVALID;
  if (!pred || !v || !target || !quad || !field || pbs < 0 || vbs < 0 || tbs < 0 || fbs < 0) return GNCA_ERR_INVALID;
  return launch_tap_curvature(kind, d, pred, (size_t)pbs, v, (size_t)vbs, target, (long)tbs, losses, dlosses, quad,
                              field, (size_t)fbs, nullptr, reinterpret_cast<hipStream_t>(hip_stream));
}

extern "C" int gnca_loss_tangent(int32_t kind, const gnca_masked_loss_desc* d, int32_t num_dirs, const float* pred,
                                 int64_t pbs, const float* v, int64_t vds, int64_t vbs, const float* target,
                                 int64_t tbs, float* losses, double* dlosses, void* hip_stream) {
  if (kind != GNCA_TAP_PREMULT && kind != GNCA_TAP_MASKED) return GNCA_ERR_INVALID;
  if (!masked_desc_ok(d) || num_dirs < 1 || (num_dirs + kLossTanDirs - 1) / kLossTanDirs > 65535)
    return GNCA_ERR_INVALID;
  if (!pred || !v || !target || !dlosses || pbs < 0 || vds < 0 || vbs < 0 || tbs < 0) return GNCA_ERR_INVALID;
  return launch_tap_loss_tangent(kind, d, num_dirs, pred, (size_t)pbs, v, (size_t)vds, (size_t)vbs, target, (long)tbs,
                                 losses, dlosses, nullptr, reinterpret_cast<hipStream_t>(hip_stream));
}

extern "C" int gnca_forward_grad(const gnca_forward_grad_desc* d, void* hip_stream) {
  if (!d || d->K < 1 || d->R < 1 || d->B < 1 || !d->dlosses || !d->coef) return GNCA_ERR_INVALID;
  if (d->num_tensors < 0 || d->num_tensors > GNCA_OPTIM_MAX_TENSORS) return GNCA_ERR_INVALID;
  if (d->flags & ~(uint32_t)GNCA_FGRAD_ACCUMULATE) return GNCA_ERR_INVALID;
  if (((uintptr_t)d->dlosses & 7) || ((uintptr_t)d->coef & 7)) return GNCA_ERR_INVALID;
  int64_t chunks = 0;
  for (int i = 0; i < d->num_tensors; ++i) {
    const gnca_forward_grad_tensor& t = d->t[i];
    if (!t.g || !t.dir || t.numel < 0 || t.dir_stride < 0) return GNCA_ERR_INVALID;
    chunks += (t.numel + kOptChunk - 1) / kOptChunk;
    if (chunks > 0x7fffffffLL) return GNCA_ERR_INVALID;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
  hipLaunchKernelGGL(gnca_fgrad_coef, dim3((unsigned)d->K), dim3(kThreads), 0, st, *d);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && chunks > 0) {
    hipLaunchKernelGGL(gnca_fgrad_apply, dim3((unsigned)chunks), dim3(kThreads), 0, st, *d);
    e = hipGetLastError();
  }
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

extern "C" int gnca_rollout_tap_loss(const gnca_step_desc* desc, const gnca_rollout_sched* sched,
                                     const gnca_rollout_taps* taps, const void* tape, size_t tape_bytes,
                                     const float* x_final, float* losses, int32_t* alive_count) {
  if (!taps_ok(desc, sched, taps) || !x_final || !losses) return GNCA_ERR_INVALID;
  if (taps->kind == GNCA_TAP_MASKED && !alive_count) return GNCA_ERR_INVALID;
  // a checkpointed tape holds the anchors only: gnca_rollout_fwd_taps writes the losses instead
  if (sched->flags & GNCA_SCHED_CHECKPOINT) return GNCA_ERR_INVALID;
  TapeLayout L;
  if (!tape_layout(desc, sched, &L)) return GNCA_ERR_INVALID;
  if (!tape) return GNCA_ERR_INVALID;
  if (tape_bytes < L.bytes) return GNCA_ERR_WORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(taps->stream);
  StreamDeviceGuard dg(st);
  TapLossArgs a;
  a.m = taps->masked;   // (B, H, W are the desc's: taps_ok)
  a.T = sched->steps;
  a.tape = reinterpret_cast<const char*>(tape);
  a.slot = L.slot;
  a.sstride = (size_t)desc->C * desc->H * desc->W;
  a.x_final = x_final;
  a.tgt = taps->target; a.tbs = (long)taps->target_bstride;
  a.losses = losses; a.alive_count = alive_count;
  for (int first = 0; first < taps->n; first += GNCA_TAP_CHUNK) {
    TapChunk ch;
    ch.first = first;
    const int n = taps->n - first < GNCA_TAP_CHUNK ? taps->n - first : GNCA_TAP_CHUNK;
    for (int j = 0; j < GNCA_TAP_CHUNK; ++j) ch.step[j] = j < n ? taps->steps[first + j] : 0;
    const dim3 grid((unsigned)desc->B, (unsigned)n), block(kThreads);
    if (taps->kind == GNCA_TAP_MASKED) hipLaunchKernelGGL(gnca_tap_loss<GNCA_TAP_MASKED>, grid, block, 0, st, a, ch);
    else hipLaunchKernelGGL(gnca_tap_loss<GNCA_TAP_PREMULT>, grid, block, 0, st, a, ch);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  }
  return GNCA_OK;
}

extern "C" size_t gnca_loss_stability_workspace_bytes(int32_t B) {
  return B > 0 ? (size_t)B * sizeof(double) : 0;
}

extern "C" int gnca_loss_stability_f32(int32_t B, int32_t H, int32_t W, const float* pred, int64_t pbs,
                                       const float* target, int64_t tbs, const uint8_t* close, float* loss,
                                       float* scale, void* ws, size_t ws_bytes, void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || !pred || !target || !close || !loss || !scale || pbs < 0 || tbs < 0)
    return GNCA_ERR_INVALID;
  if (!ws || ws_bytes < gnca_loss_stability_workspace_bytes(B) || ((uintptr_t)ws & 7)) return GNCA_ERR_WORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(gnca_stability_partial, dim3(B), dim3(kThreads), 0, st, H, W, pred, (long)pbs, target,
                     (long)tbs, close, part);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    hipLaunchKernelGGL(gnca_stability_finish, dim3(1), dim3(kThreads), 0, st, B, H, W, close, part, loss, scale);
    e = hipGetLastError();
  }
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

extern "C" int gnca_loss_stability_bwd_f32(int32_t B, int32_t H, int32_t W, const float* pred, int64_t pbs,
                                           const float* target, int64_t tbs, const uint8_t* close,
                                           const float* scale, const float* g, float* grad_pred, int64_t gbs,
                                           void* stream) {
  if (B <= 0 || H <= 0 || W <= 0 || !pred || !target || !close || !scale || !g || !grad_pred || pbs < 0 ||
      tbs < 0 || gbs < 0)
    return GNCA_ERR_INVALID;
  hipLaunchKernelGGL(gnca_stability_bwd, dim3(elementwise_blocks((size_t)B * 4 * H * W)), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), B, H, W, pred, (long)pbs, target, (long)tbs, close, scale,
                     g, grad_pred, (long)gbs);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

extern "C" int gnca_damage_f32(const gnca_damage_desc* d, float* state, const int32_t* pos,
                               const float* noise, void* stream) {
  if (!d || !state || d->B <= 0 || d->C < 4 || d->H <= 0 || d->W <= 0) return GNCA_ERR_INVALID;
  if (d->kind < GNCA_DMG_SQUARE || d->kind > GNCA_DMG_HIDDEN_NOISE) return GNCA_ERR_INVALID;
  const bool geo = d->kind == GNCA_DMG_SQUARE || d->kind == GNCA_DMG_CIRCLE || d->kind == GNCA_DMG_STRIPE_H ||
                   d->kind == GNCA_DMG_STRIPE_V || d->kind == GNCA_DMG_GAUSSIAN;
  if (geo && !pos) return GNCA_ERR_INVALID;
  if (!geo && !noise) return GNCA_ERR_INVALID;
  if (d->kind == GNCA_DMG_HIDDEN_NOISE && d->C <= 4) return GNCA_OK;
  const size_t cells = (size_t)d->B * d->H * d->W;
  size_t blocks = (cells + kThreads - 1) / kThreads;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(gnca_damage, dim3((unsigned)blocks), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), *d, state, pos, noise);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    g_last_hip = (int)e;
    return GNCA_ERR_HIP;
  }
  return GNCA_OK;
}

extern "C" int gnca_damage_policy(const gnca_damage_policy_desc* d, float* state, const int32_t* forced_kind,
                                  const int64_t* event_dev, int32_t* draws_out, float* noise_out) {
  if (!d || !state || d->B < 0 || d->C < 4 || d->H <= 0 || d->W <= 0) return GNCA_ERR_INVALID;
  if (d->scope != GNCA_DMG_SCOPE_BATCH && d->scope != GNCA_DMG_SCOPE_SAMPLE) return GNCA_ERR_INVALID;
  if (d->n_kinds < 1 || d->n_kinds > GNCA_DMG_MAX_KINDS || d->size_max < d->size_min) return GNCA_ERR_INVALID;
  for (int k = 0; k < d->n_kinds; ++k)
    if (d->kinds[k] < GNCA_DMG_SQUARE || d->kinds[k] > GNCA_DMG_STRIPES_AUTO) return GNCA_ERR_INVALID;
  if (d->B == 0) return GNCA_OK;
  const bool vec = d->W % 4 == 0 && ((uintptr_t)state & 15) == 0 && ((uintptr_t)noise_out & 15) == 0;
  const int vpr = vec ? d->W / 4 : d->W;               // vectors per row
  int band_rows = (kThreads + vpr - 1) / vpr;          // about one vector per thread and channel
  if (band_rows > d->H) band_rows = d->H;
  const int nbands = (d->H + band_rows - 1) / band_rows;
  if ((long)d->B * nbands > 0x7fffffffL) return GNCA_ERR_INVALID;
  const dim3 grid((unsigned)((long)d->B * nbands));
  hipStream_t st = reinterpret_cast<hipStream_t>(d->stream);
  if (vec)
    hipLaunchKernelGGL(gnca_damage_policy_k<4>, grid, dim3(kThreads), 0, st, *d, band_rows, nbands, state, forced_kind,
                       event_dev, draws_out, noise_out);
  else
    hipLaunchKernelGGL(gnca_damage_policy_k<1>, grid, dim3(kThreads), 0, st, *d, band_rows, nbands, state, forced_kind,
                       event_dev, draws_out, noise_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    g_last_hip = (int)e;
    return GNCA_ERR_HIP;
  }
  return GNCA_OK;
}

extern "C" size_t gnca_image_metrics_workspace_bytes(int32_t N, int32_t H, int32_t W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  const int nb = met_bands(N, H);
  return nb > 1 ? (size_t)N * nb * 4 * sizeof(double) : 0;
}

extern "C" int gnca_image_metrics_f32(int32_t N, int32_t H, int32_t W, const float* pred, int64_t pbs,
                                      const float* target, int64_t tbs, float* out, void* ws, size_t ws_bytes,
                                      void* stream) {
  if (N <= 0 || H <= 0 || W <= 0 || !pred || !target || !out || pbs < 0 || tbs < 0) return GNCA_ERR_INVALID;
  const int nb = met_bands(N, H);
  if (nb == 0) return GNCA_ERR_INVALID;
  const size_t need = nb > 1 ? (size_t)N * nb * 4 * sizeof(double) : 0;
  if (need && (!ws || ws_bytes < need || ((uintptr_t)ws & 7))) return GNCA_ERR_WORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(gnca_image_metrics, dim3((unsigned)(N * nb)), dim3(kThreads), 0, st, nb, H, W, pred, (long)pbs,
                     target, (long)tbs, part, out);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && nb > 1) {
    hipLaunchKernelGGL(gnca_image_metrics_finish, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       st, N, nb, H, W, part, out);
    e = hipGetLastError();
  }
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}

extern "C" size_t gnca_state_vitals_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
  if (B <= 0 || C < 4 || H <= 0 || W <= 0) return 0;
  int nbands, nchunks;
  return (size_t)B * (size_t)vit_tiles(B, H, W, &nbands, &nchunks) * kVitF * sizeof(double);
}

extern "C" int gnca_state_vitals(int32_t B, int32_t C, int32_t H, int32_t W, const float* x, int64_t x_bstride,
                                 float alpha_thr, double* out, void* ws, size_t ws_bytes, void* stream) {
  if (B <= 0 || C < 4 || H <= 0 || W <= 0 || !x || !out || x_bstride < 0 || ((uintptr_t)out & 7))
    return GNCA_ERR_INVALID;
  int nbands, nchunks;
  const long np = vit_tiles(B, H, W, &nbands, &nchunks);
  if (np == 0) return GNCA_ERR_INVALID;
  if (!ws || ws_bytes < (size_t)B * (size_t)np * kVitF * sizeof(double) || ((uintptr_t)ws & 7))
    return GNCA_ERR_WORKSPACE;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>(ws);
  const dim3 grid((unsigned)(np * B));
  // four cells per thread where W % 4 == 0 (a function of the shape: the sums' order), as one 16-byte
  // load where every address is 16-byte aligned
  const bool aligned = x_bstride % 4 == 0 && ((uintptr_t)x & 15) == 0;
  auto kern = W % 4 != 0 ? gnca_state_vitals_k<1, true>
                         : (aligned ? gnca_state_vitals_k<4, true> : gnca_state_vitals_k<4, false>);
  hipLaunchKernelGGL(kern, grid, dim3(kThreads), 0, st, C, H, W, nbands, nchunks, x, (long)x_bstride, alpha_thr,
                     part);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    constexpr int per = kThreads / 64;   // samples per finish workgroup
    hipLaunchKernelGGL(gnca_state_vitals_finish, dim3((unsigned)((B + per - 1) / per)), dim3(kThreads), 0, st, B, C,
                       H, W, (int)np, part, out);
    e = hipGetLastError();
  }
  if (e != hipSuccess) { g_last_hip = (int)e; return GNCA_ERR_HIP; }
  return GNCA_OK;
}
