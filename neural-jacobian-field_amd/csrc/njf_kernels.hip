// Fused HIP kernels + C ABI (include/njf_hip.h) for the NJF volumetric-rendering hot path.
// gfx950 only.  Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC
// (-ffp-contract=off: geometry must round exactly like the ATen ops of the reference path;
//  every intended fma is written as fmaf()).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "../../include/njf_hip.h"
#include "njf_device.h"

// =============================================================================================
// error codes
// =============================================================================================
enum {
  NJF_OK = 0,
  NJF_E_NULL = -1,
  NJF_E_SHAPE = -2,
  NJF_E_ACTION_DIM = -3,
  NJF_E_SAMPLES = -4,
  NJF_E_DOUT = -5,
  NJF_E_MODE = -6,
  NJF_E_GMAP = -7,
  NJF_E_VALUE = -8,
};

extern "C" int njf_abi_version(void) { return NJF_ABI_VERSION; }
extern "C" int njf_rays_per_workgroup(void) { return NJF_WAVES; }

extern "C" const char* njf_error_string(int code) {
  switch (code) {
    case NJF_OK: return "ok";
    case NJF_E_NULL: return "required pointer is NULL";
    case NJF_E_SHAPE: return "invalid shape (negative/zero extent or overflow)";
    case NJF_E_ACTION_DIM: return "action_dim must be in [1, NJF_MAX_ACTION_DIM]";
    case NJF_E_SAMPLES: return "samples per ray must be in [1, 256] for the proposal pass / >= 1 for rendering";
    case NJF_E_DOUT: return "ResnetFC d_out must be in [1, 32]";
    case NJF_E_MODE: return "unknown mode";
    case NJF_E_GMAP: return "feature map stride/offset does not cover NJF_ZDIM channels or is not 16-byte aligned";
    case NJF_E_VALUE:
      return "invalid option value (solver: beta must be > 0, reg and damping >= 0; mesh: every grid dimension >= 2, a finite "
             "threshold, capacities >= 0, a known phase)";
    default: return code > 0 ? "HIP runtime error (hipError_t)" : "unknown njf error";
  }
}

static inline bool valid_base_precision(int p) {
  return p == NJF_PRECISION_F32 || p == NJF_PRECISION_F16X2 || p == NJF_PRECISION_F16F6 || p == NJF_PRECISION_F16;
}
// `precision` of the decoder entry points may name a second precision for the Jacobian head: NJF_PRECISION_MIXED(d, j)
static inline int density_precision(int p) { return p & 15; }
static inline int jacobian_precision(int p) { return (p >> 4) ? (p >> 4) - 1 : (p & 15); }
static inline bool valid_precision(int p) {
  if (p < 0 || p > 0xff || !valid_base_precision(density_precision(p)) || !valid_base_precision(jacobian_precision(p))) return false;
  const int d = density_precision(p), j = jacobian_precision(p);
  // d = j has ONE code, the plain value: NJF_PRECISION_MIXED(d, d) is refused, so that every accepted code is one a caller can
  // have meant.  Mixed forms: the two split-precision modes in either order (the plain-fp16 mode reads an fp16 map: never mixed)
  if (d == j) return (p >> 4) == 0;
  return d != NJF_PRECISION_F32 && j != NJF_PRECISION_F32 && d != NJF_PRECISION_F16 && j != NJF_PRECISION_F16;
}

static inline int launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? NJF_OK : (int)e;
}

// =============================================================================================
// weight packing
// =============================================================================================
struct PackLayer {
  const float* w;  // [d_out, d_in] row-major (torch Linear)
  const float* b;  // [d_out] or NULL
  int d_out, d_in;
  int mb, kb;  // output / input 32-blocks
  int kind;    // 0 plain, 1 lin_in (PE slots + bias column), 2 colour layer 0 (geo|1|sh slots), 3 transposed (backward chain)
  int prec;    // NJF_PRECISION_*
  float* dst;  // kb*4*mb*256 floats (same byte count in both precisions)
  float* bdst;  // 32*mb floats (logical order, zero padded) or NULL
  int bias_form;  // 0: fp32 values; 1: each entry the bit pattern of {fp16 hi, fp16 lo} of the bias (bias = hi + lo to 22 bits):
                  //    the A operand of the plain-fp16 networks' bias MFMA (njf_device.h: bias_init); 2: zeros (the bias lives elsewhere)
};

// logical (row f, input slot k) -> source value
__device__ __forceinline__ float pack_source(const PackLayer& L, int f, int k) {
  if (f >= L.d_out) return 0.f;
  if (L.kind == 0) return k < L.d_in ? L.w[f * L.d_in + k] : 0.f;
  if (L.kind == 1) {  // slots: [sin 0..29 | x | y || cos 30..59 | z | bias]
    int ch;
    if (k < 30) ch = k;
    else if (k == 30) ch = 60;
    else if (k == 31) ch = 61;
    else if (k < 62) ch = k - 2;
    else if (k == 62) ch = 62;
    else ch = -1;
    return ch >= 0 ? L.w[f * L.d_in + ch] : L.b[f];
  }
  if (L.kind == 3) return k < L.d_in ? L.w[k * L.d_out + f] : 0.f;  // transposed layer: row f of W^T, W stored [d_in, d_out]
  // slots: [geo 0..14 | bias || sh 0..15]
  if (k < 15) return L.w[f * L.d_in + k];
  if (k == 15) return L.b[f];
  return L.w[f * L.d_in + (k - 1)];
}


__device__ __forceinline__ float pack_bias_entry(const PackLayer& L, int f) {
  const float b = (f < L.d_out && L.b) ? L.b[f] : 0.f;
  if (L.bias_form == 2) return 0.f;
  if (L.bias_form == 1) {
    const _Float16 hi = (_Float16)b;
    const _Float16 lo = (_Float16)(b - (float)hi);
    return __uint_as_float((unsigned)__builtin_bit_cast(unsigned short, hi) | ((unsigned)__builtin_bit_cast(unsigned short, lo) << 16));
  }
  return b;
}

// fp6 e2m3 (1 sign, 2 exponent bits with bias 1, 3 mantissa bits; max 7.5, subnormal step 1/8), round to nearest even,
// saturating: the value set of v_mfma_scale_*_f8f6f4 with cbsz/blgp = 2.
__device__ __forceinline__ unsigned encode_e2m3(float v) {
  const unsigned sign = v < 0.f ? 32u : 0u;
  const float a = fminf(fabsf(v), 7.5f);
  unsigned code;
  if (a < 1.0f) {
    code = (unsigned)rintf(a * 8.0f);  // 0..8: 8 is the encoding of 1.0 (exponent field 1, mantissa 0)
  } else {
    int e = a >= 4.0f ? 2 : (a >= 2.0f ? 1 : 0);
    float q = rintf(a * (8.0f / (float)(1 << e)));  // 8..16
    if (q >= 16.0f) {
      q = 8.0f;
      e += 1;
    }
    code = ((unsigned)(e + 1) << 3) | ((unsigned)q - 8u);
    if (e > 2) code = 31u;
  }
  return sign | code;
}

// PREC_F16F6 form of a 128-output layer (mb = 4): one 32 KiB chunk per K-range of 64 (njf_device.h: F6_* offsets).
__device__ __forceinline__ void pack_layer_f16f6_body(const PackLayer& L) {
  const int chunks = L.kb >> 1;
  _Float16* dst16 = (_Float16*)L.dst;
  // (a) hi fp16 fragments [chunk][t][m][lane][8]
  const int n = chunks * 4 * 4 * 512;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int i8 = i & 7, lane = (i >> 3) & 63;
    int rest = i >> 9;
    const int m = rest & 3;
    rest >>= 2;
    const int t = rest & 3, c = rest >> 2;
    const int ip = lane & 31, kh = lane >> 5;
    const int f = 16 * L.mb * ((ip >> 2) & 1) + 16 * m + (ip & 3) + 4 * (ip >> 3);
    const int k = 16 * L.kb * kh + 32 * c + 8 * t + i8;
    dst16[(size_t)c * (2 * NJF_CHUNK_FLOATS) + (F6_HI >> 1) + ((t * 4 + m) * 64 + lane) * 8 + i8] = (_Float16)pack_source(L, f, k);
  }
  // (b) fp6 fragments + scales: one thread per (chunk, m, w, lane)
  const int nf = chunks * 4 * 2 * 64;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nf; i += gridDim.x * blockDim.x) {
    const int lane = i & 63, w = (i >> 6) & 1, m = (i >> 7) & 3, c = i >> 9;
    const int ip = lane & 31, kh = lane >> 5;
    const int f = 16 * L.mb * ((ip >> 2) & 1) + 16 * m + (ip & 3) + 4 * (ip >> 3);
    float v[32], amax = 0.f;
#pragma unroll
    for (int e = 0; e < 32; ++e) {
      const float x = pack_source(L, f, 16 * L.kb * kh + 32 * c + e);
      const float hi = (float)(_Float16)x;
      v[e] = w == 0 ? hi : (float)(_Float16)(x - hi);  // the residual as the f16x2 path holds it
      amax = fmaxf(amax, fabsf(v[e]));
    }
    int ex = amax > 0.f ? ilogbf(amax) - 2 : -126;   // largest element lands in [4, 8) (clamped at 7.5)
    ex = max(ex, -126);
    const float inv = ldexpf(1.0f, -ex);
    unsigned words[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 32; ++e) {
      const unsigned long long code = encode_e2m3(v[e] * inv);
      const int bit = 6 * e;
      words[bit >> 5] |= (unsigned)(code << (bit & 31));
      if ((bit & 31) > 26) words[(bit >> 5) + 1] |= (unsigned)(code >> (32 - (bit & 31)));
    }
    char* base = (char*)L.dst + (size_t)c * (NJF_CHUNK_FLOATS * 4);
    unsigned* p1 = (unsigned*)(base + F6_P1 + ((2 * m + w) * 64 + lane) * 16);
    unsigned* p2 = (unsigned*)(base + F6_P2 + ((2 * m + w) * 64 + lane) * 8);
    p1[0] = words[0];
    p1[1] = words[1];
    p1[2] = words[2];
    p1[3] = words[3];
    p2[0] = words[4];
    p2[1] = words[5];
    ((unsigned char*)(base + F6_SCALE + w * 256 + lane * 4))[m] = (unsigned char)(ex + 127);
  }
  // (c) the unused tail of every chunk (the weight DMA moves whole chunks)
  const int tail = (NJF_CHUNK_FLOATS * 4 - (F6_SCALE + 512)) >> 2;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < chunks * tail; i += gridDim.x * blockDim.x)
    ((unsigned*)((char*)L.dst + (size_t)(i / tail) * (NJF_CHUNK_FLOATS * 4) + F6_SCALE + 512))[i % tail] = 0u;
  if (L.bdst != nullptr && blockIdx.x == 0) {
    for (int f = threadIdx.x; f < 32 * L.mb; f += blockDim.x) L.bdst[f] = pack_bias_entry(L, f);
  }
}

__global__ void pack_layer_f16f6_kernel(PackLayer L) { pack_layer_f16f6_body(L); }

__device__ __forceinline__ void pack_layer_body(const PackLayer& L) {
  if (L.prec == NJF_PRECISION_F32) {
    const int n = L.kb * 4 * L.mb * 256;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
      const int e = i & 3, lane = (i >> 2) & 63;
      int rest = i >> 8;
      const int m = rest % L.mb;
      rest /= L.mb;
      const int q = rest & 3, kb = rest >> 2;
      const int ip = lane & 31, kh = lane >> 5;
      const int f = 16 * L.mb * ((ip >> 2) & 1) + 16 * m + (ip & 3) + 4 * (ip >> 3);  // logical output row
      const int k = 16 * L.kb * kh + 16 * kb + 4 * q + e;                              // logical input slot
      L.dst[i] = pack_source(L, f, k);
    }
  } else if (L.prec == NJF_PRECISION_F16) {
    // [t][m][lane][8 x f16]: ONE fp16 per weight (half the bytes of the other forms; the rest of the layer's slot is unused)
    _Float16* dst = (_Float16*)L.dst;
    const int n = L.kb * 2 * L.mb * 512;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
      const int i8 = i & 7, lane = (i >> 3) & 63;
      const int rest = i >> 9;
      const int m = rest % L.mb, t = rest / L.mb;
      const int ip = lane & 31, kh = lane >> 5;
      const int f = 16 * L.mb * ((ip >> 2) & 1) + 16 * m + (ip & 3) + 4 * (ip >> 3);
      const int k = 16 * L.kb * kh + 8 * t + i8;
      dst[(size_t)(t * L.mb + m) * 512 + lane * 8 + i8] = (_Float16)pack_source(L, f, k);
    }
  } else {
    // [t][m][hi|lo][lane][8 x f16]; lane half kh supplies the 8 k-values 16*KB*kh + 8*t + i of K-step t
    _Float16* dst = (_Float16*)L.dst;
    const int n = L.kb * 2 * L.mb * 512;  // (t, m, lane, i8) tuples; each writes its hi and lo plane entry
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
      const int i8 = i & 7, lane = (i >> 3) & 63;
      const int rest = i >> 9;
      const int m = rest % L.mb, t = rest / L.mb;
      const int ip = lane & 31, kh = lane >> 5;
      const int f = 16 * L.mb * ((ip >> 2) & 1) + 16 * m + (ip & 3) + 4 * (ip >> 3);
      const int k = 16 * L.kb * kh + 8 * t + i8;
      const float v = pack_source(L, f, k);
      const _Float16 hi = (_Float16)v;
      const _Float16 lo = (_Float16)(v - (float)hi);
      const size_t o = ((size_t)(t * L.mb + m) * 2) * 512 + lane * 8 + i8;
      dst[o] = hi;
      dst[o + 512] = lo;
    }
  }
  if (L.bdst != nullptr && blockIdx.x == 0) {
    for (int f = threadIdx.x; f < 32 * L.mb; f += blockDim.x) L.bdst[f] = pack_bias_entry(L, f);
  }
}

__global__ void pack_layer_kernel(PackLayer L) { pack_layer_body(L); }

// Several layers in ONE launch (blockIdx.y = layer): a network's pack is 11-22 layers of a few microseconds each, and an optimiser
// step re-packs every network it touched -- forward blobs and the backward chain's transposed blobs (an action-mode step with the
// transformer head: 36 pack launches; a perception step: ~70).  The njf_pack_* entry points queue their layers (PackScope) and
// flush once; every layer writes its own destination, so the order among them does not matter.
#define NJF_PACK_BATCH 24
struct PackBatch {
  PackLayer l[NJF_PACK_BATCH];
  unsigned char f6[NJF_PACK_BATCH];   // 1: the fp6-corrected chunk form (pack_layer_f16f6_body)
  int count;
};

__global__ void pack_batch_kernel(PackBatch B) {
  const int k = blockIdx.y;
  if (B.f6[k]) pack_layer_f16f6_body(B.l[k]);
  else pack_layer_body(B.l[k]);
}

__global__ void fill_kernel(float* p, int n, float v) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = v;
}

// position of logical feature f inside its 32*MB-channel block of the hoisted map.  Two layouts, one per gather form of
// add_hoisted_latent (njf_device.h); a network's layout follows its MFMA precision:
//   0 "half" (F32, F16X2): the two lanes that own a point read adjacent 16-byte pieces
//   1 "quad" (F16F6): the 16*MB floats of a lane are contiguous, accumulator register 4*e + i <-> piece i, dword e
//   2 "half, fp16 map" (F16): as 0 with 8-channel pieces
__host__ __device__ inline int njf_hoist_layout(int precision) {
  return precision == NJF_PRECISION_F16F6 ? 1 : (precision == NJF_PRECISION_F16 ? 2 : 0);
}
__host__ __device__ inline int njf_hoist_position(int f, int mb_count, int layout) {
  const int hh = f / (16 * mb_count), r = f % (16 * mb_count);
  const int m = r >> 4;
  if (layout == 0) {
    const int q = (r >> 2) & 3, e = r & 3;
    return 32 * m + 8 * q + 4 * hh + e;
  }
  if (layout == 2) {  // fp16 map: 16-byte pieces of 8 channels, the two lane halves adjacent (add_hoisted_latent_f16)
    const int q = (r >> 3) & 1, e = r & 7;
    return 32 * m + 16 * q + 8 * hh + e;
  }
  const int e = (r >> 2) & 3, i = r & 3;
  return 16 * mb_count * hh + 16 * m + 4 * i + e;
}

// the same function for callers that write hoisted channels themselves (per-image biases, folded projections)
extern "C" int njf_hoisted_channel(int feature, int block_channels, int precision) {
  if (block_channels < 32 || (block_channels & 31) || feature < 0 || feature >= block_channels) return NJF_E_SHAPE;
  if (!valid_base_precision(precision)) return NJF_E_MODE;
  return njf_hoist_position(feature, block_channels / 32, njf_hoist_layout(precision));
}

// lin_z.{0,1,2}.weight [128,512] -> wz[k * ld + 128*i + pos(f)]  (k-major: coalesced B operand of the projection)
// fold0 / fold1 (plain-fp16 networks): fc_1.bias of blocks 0 / 1, added to the map bias of blocks 1 / 2 -- the latent of block
// k + 1 is added to h right behind block k's  h += fc_1(...) + b_1, and the bilinear weights of a footprint sum to 1, so
// bilerp(G + b_1) = bilerp(G) + b_1: those two bias additions cost nothing in the kernel
__global__ void pack_linz_kernel(const float* w0, const float* w1, const float* w2, const float* b0, const float* b1,
                                 const float* b2, float* wz, int ld, float* bz, int layout, const float* fold0,
                                 const float* fold1) {
  const int n = 3 * 128 * 512;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int c = i % 384, k = i / 384;
    const int l = c >> 7, f = c & 127;
    const float* w = l == 0 ? w0 : (l == 1 ? w1 : w2);
    wz[(size_t)k * ld + 128 * l + njf_hoist_position(f, 4, layout)] = w[f * 512 + k];
  }
  if (blockIdx.x == 0)
    for (int c = threadIdx.x; c < 384; c += blockDim.x) {
      const int l = c >> 7, f = c & 127;
      const float extra = l == 1 ? (fold0 ? fold0[f] : 0.f) : (l == 2 ? (fold1 ? fold1[f] : 0.f) : 0.f);
      bz[128 * l + njf_hoist_position(f, 4, layout)] = (l == 0 ? b0 : (l == 1 ? b1 : b2))[f] + extra;
    }
}

// The layers an entry point packs, launched together when the scope ends (also on an early error return).  One scope per entry
// point call, on the calling thread (the C ABI is re-entrant: the queue lives in the scope object, the pointer to it is thread-local).
struct PackScope;
static thread_local PackScope* g_pack_scope = nullptr;
struct PackScope {
  PackBatch b;
  hipStream_t s;
  explicit PackScope(hipStream_t stream) : s(stream) {
    b.count = 0;
    g_pack_scope = this;
  }
  void flush() {
    if (b.count > 0) pack_batch_kernel<<<dim3(64, b.count), 256, 0, s>>>(b);
    b.count = 0;
  }
  void add(const PackLayer& L, bool f6) {
    if (b.count == NJF_PACK_BATCH) flush();
    b.l[b.count] = L;
    b.f6[b.count] = f6 ? 1 : 0;
    ++b.count;
  }
  ~PackScope() {
    flush();
    g_pack_scope = nullptr;
  }
  PackScope(const PackScope&) = delete;
  PackScope& operator=(const PackScope&) = delete;
};

static void launch_pack(const float* w, const float* b, int d_out, int d_in, int mb, int kb, int kind, int prec, float* dst,
                        float* bdst, hipStream_t s, int bias_form = 0) {
  PackLayer L{w, b, d_out, d_in, mb, kb, kind, prec, dst, bdst, bias_form};
  const int n = kb * 4 * mb * 256;
  bool f6 = false;
  if (prec == NJF_PRECISION_F16F6) {
    // the 128-wide layers take the fp6-corrected chunk form; narrow layers keep the F16X2 form (njf_device.h: mma_chunk)
    if (mb == 4 && (kb & 1) == 0) f6 = true;
    else L.prec = NJF_PRECISION_F16X2;
  }
  if (g_pack_scope != nullptr && g_pack_scope->s == s) {
    g_pack_scope->add(L, f6);
    return;
  }
  if (f6) pack_layer_f16f6_kernel<<<64, 256, 0, s>>>(L);
  else pack_layer_kernel<<<(n + 255) / 256, 256, 0, s>>>(L);
}

extern "C" int njf_pack_resnetfc_ld(const NjfResnetFcWeights* src, float* w_out, float* b_out, float* wz_out, int wz_ld,
                                    float* bz_out, int precision, void* stream) {
  if (!src || !w_out || !b_out) return NJF_E_NULL;
  if (!valid_base_precision(precision)) return NJF_E_MODE;
  const int P = precision;
  if (src->d_out < 1 || src->d_out > 32) return NJF_E_DOUT;
  if (!src->lin_in_w || !src->lin_in_b || !src->lin_out_w || !src->lin_out_b) return NJF_E_NULL;
  for (int i = 0; i < 5; ++i)
    if (!src->fc0_w[i] || !src->fc0_b[i] || !src->fc1_w[i] || !src->fc1_b[i]) return NJF_E_NULL;
  if (P == NJF_PRECISION_F16 && !wz_out) return NJF_E_NULL;  // two of its accumulated biases live in the hoisted map's bias
  hipStream_t s = (hipStream_t)stream;
  PackScope scope(s);   // the network's 12 layers: one launch
  // chunk 0: lin_in 63(+bias) -> 128
  launch_pack(src->lin_in_w, src->lin_in_b, 128, NJF_PE_DIM, 4, 2, 1, P, w_out, nullptr, s);
  // a 128 x 128 layer is two chunks (K = 64 each), one in the plain-fp16 form: NJF_RESNET_CHUNKS_F16 = 12 of the blob's 22 slots
  const int per_layer = P == NJF_PRECISION_F16 ? 1 : 2;
  for (int i = 0; i < 5; ++i) {
    float* base = w_out + (size_t)(1 + 2 * per_layer * i) * NJF_CHUNK_FLOATS;
    launch_pack(src->fc0_w[i], src->fc0_b[i], 128, 128, 4, 4, 0, P, base, b_out + 256 * i, s);
    // plain-fp16 networks: fc_1.bias of blocks 0, 1 is folded into the hoisted map (pack_linz_kernel), the others are stored
    // as {hi, lo} fp16 pairs for the bias MFMA
    const int bias_form = P == NJF_PRECISION_F16 ? (i < 2 ? 2 : 1) : 0;
    launch_pack(src->fc1_w[i], src->fc1_b[i], 128, 128, 4, 4, 0, P, base + per_layer * NJF_CHUNK_FLOATS, b_out + 256 * i + 128, s,
                bias_form);
  }
  float* last = w_out + (size_t)(1 + 10 * per_layer) * NJF_CHUNK_FLOATS;
  launch_pack(src->lin_out_w, src->lin_out_b, src->d_out, 128, 1, 4, 0, P, last, b_out + 1280, s);
  fill_kernel<<<16, 256, 0, s>>>(last + 4096, 4096, 0.f);
  if (wz_out) {
    if (!bz_out || wz_ld < 384) return NJF_E_SHAPE;
    for (int i = 0; i < 3; ++i)
      if (!src->lin_z_w[i] || !src->lin_z_b[i]) return NJF_E_NULL;
    pack_linz_kernel<<<256, 256, 0, s>>>(src->lin_z_w[0], src->lin_z_w[1], src->lin_z_w[2], src->lin_z_b[0],
                                         src->lin_z_b[1], src->lin_z_b[2], wz_out, wz_ld, bz_out, njf_hoist_layout(P),
                                         P == NJF_PRECISION_F16 ? src->fc1_b[0] : nullptr,
                                         P == NJF_PRECISION_F16 ? src->fc1_b[1] : nullptr);
  }
  scope.flush();   // (before the status query: a failed batch launch must be this call's error)
  return launch_status();
}

extern "C" int njf_pack_resnetfc(const NjfResnetFcWeights* src, float* w_out, float* b_out, float* wz_out, float* bz_out,
                                 int precision, void* stream) {
  return njf_pack_resnetfc_ld(src, w_out, b_out, wz_out, 384, bz_out, precision, stream);
}

extern "C" int njf_pack_linear(const float* w, const float* b, int d_out, int d_in, int kind, float* w_out, float* b_out,
                               int precision, void* stream) {
  if (!w || !w_out) return NJF_E_NULL;
  if (!valid_base_precision(precision)) return NJF_E_MODE;
  if (d_out < 1 || d_in < 1) return NJF_E_SHAPE;
  if (kind == 1 && (d_in != NJF_PE_DIM || !b)) return NJF_E_SHAPE;
  if (kind != 0 && kind != 1) return NJF_E_MODE;
  const int mb = (d_out + 31) / 32, kb = kind == 1 ? 2 : (d_in + 31) / 32;
  launch_pack(w, b, d_out, d_in, mb, kb, kind, precision, w_out, b_out, (hipStream_t)stream);
  return launch_status();
}

extern "C" int njf_pack_color_head(const NjfColorHeadWeights* src, float* w_out, float* b_out, int precision,
                                   void* stream) {
  if (!src || !w_out || !b_out || !src->w0 || !src->b0 || !src->w1 || !src->b1 || !src->w2 || !src->b2) return NJF_E_NULL;
  if (!valid_base_precision(precision)) return NJF_E_MODE;
  hipStream_t s = (hipStream_t)stream;
  PackScope scope(s);
  launch_pack(src->w0, src->b0, 64, 31, 2, 1, 2, precision, w_out, nullptr, s);
  launch_pack(src->w1, src->b1, 64, 64, 2, 2, 0, precision, w_out + 2048, b_out, s);
  launch_pack(src->w2, src->b2, 3, 64, 1, 2, 0, precision, w_out + 6144, b_out + 64, s);
  scope.flush();   // (before the status query: a failed batch launch must be this call's error)
  return launch_status();
}

// =============================================================================================
// feature projection  G[b,p,n] = sum_k F[b,k,p] * wz[k*ld+n] + bz[n]   (exact-fp32 MFMA kernel; split variant below)
// =============================================================================================

// Split-precision variant (PREC_F16X2): one wave = 64 texels (two A tiles) x 32*NJF_PROJ_NT channels, K swept 16
// at a time with v_mfma_f32_32x32x16_f16.  Both operands are fp32 in memory and split x = hi + lo on the fly
// (hi*hi + hi*lo + lo*hi, fp32 accumulate: same accuracy class as the fp32 kernel at 3/16 of its matrix time).
// Lane (j, kh) supplies k = 16*t + 8*kh .. +7 of texel row j (A) / output channel column j (B).
__device__ __forceinline__ void split8(const float (&x)[8], f16x8& hi, f16x8& lo) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const _Float16 h = (_Float16)x[i];
    hi[i] = h;
    lo[i] = (_Float16)(x[i] - (float)h);
  }
}

// Workgroup tile 128 texels x 128 channels, K swept 16 at a time.  Per step every thread fetches 8 k-values of ONE texel
// (A) and of ONE channel (B) from global memory -- both coalesced across the threads -- splits them ONCE into fp16 hi/lo and
// writes them to LDS as ready MFMA fragments ([hi|lo][32-row block][lane][8 x f16]: conflict-free 16-byte writes and
// reads); each of the four waves then computes a 64 x 64 sub-tile from 8 fragment reads and 12 MFMAs.  Double-buffered:
// the next step's global loads are in flight during the MFMAs, one barrier per step.  (The round-1 form had every wave
// fetch and split its own operands straight from global memory: 32 load instructions per 12 MFMAs, the feature plane
// re-read once per 64 output channels -- 13 % matrix-pipe efficiency; products and their order are unchanged, results are
// bit-identical.)
typedef unsigned u32x4p __attribute__((ext_vector_type(4)));
// KS = k-values per step: 16 is shipped (C2, both maps of a frame: 0.127 -> 0.102 ms against the round-1 form; a 32-wide
// step, twice the LDS and half the barriers, measured 0.117 ms).
// OUT16: the result (bias added in fp32) is rounded ONCE to fp16 and stored as a [.., n] map of halves -- the hoisted map of
// the plain-fp16 networks (NJF_PRECISION_F16); the products themselves stay error-compensated.
template <int KS, bool OUT16 = false>
__global__ void __launch_bounds__(256, 2) project_kernel_f16x2(const float* __restrict__ feats, const float* __restrict__ wz,
                                                            const float* __restrict__ bz, int hw, int n, int ld, int K,
                                                            float* __restrict__ out) {
  constexpr int NS = KS / 16;               // 16-wide sub-steps per step
  __shared__ u32x4p s_a[2][NS][2][4][64];   // [stage][sub-step][hi|lo][32-texel block][lane]
  __shared__ u32x4p s_b[2][NS][2][4][64];   // [stage][sub-step][hi|lo][32-channel block][lane]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, kh = lane >> 5;
  const int b = blockIdx.z;
  const int p0 = blockIdx.x * 128, n0 = blockIdx.y * 128;
  // loader role: row `lr` of the tile (a texel for A, a channel for B), k-group `lk` (8 consecutive k of a sub-step's 16)
  const int lr = tid & 127, lk = tid >> 7;
  const float* fa = feats + (size_t)b * K * hw + min(p0 + lr, hw - 1);
  const float* fb = wz + min(n0 + lr, n - 1);
  const int blk = lr >> 5, slot = lk * 32 + (lr & 31);
  // compute role: wave (wm, wn) owns texel blocks 2*wm, 2*wm+1 and channel blocks 2*wn, 2*wn+1
  const int wm = wave & 1, wn = wave >> 1;
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[a][t] = (f32x16)(0.f);
  float xa[NS][8], xb[NS][8];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int kb = k0 + 16 * u + 8 * lk;
#pragma unroll
      for (int i = 0; i < 8; ++i) xa[u][i] = fa[(size_t)(kb + i) * hw];
#pragma unroll
      for (int i = 0; i < 8; ++i) xb[u][i] = fb[(size_t)(kb + i) * ld];
    }
  };
  fetch(0);
  int st = 0;
  for (int k0 = 0; k0 < K; k0 += KS, st ^= 1) {
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      f16x8 h, l;
      split8(xa[u], h, l);
      s_a[st][u][0][blk][slot] = __builtin_bit_cast(u32x4p, h);
      s_a[st][u][1][blk][slot] = __builtin_bit_cast(u32x4p, l);
      split8(xb[u], h, l);
      s_b[st][u][0][blk][slot] = __builtin_bit_cast(u32x4p, h);
      s_b[st][u][1][blk][slot] = __builtin_bit_cast(u32x4p, l);
    }
    __syncthreads();  // stage `st` complete; every wave has finished reading the other stage (it did so before this barrier)
    if (k0 + KS < K) fetch(k0 + KS);
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      f16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        ah[a] = __builtin_bit_cast(f16x8, s_a[st][u][0][2 * wm + a][lane]);
        al[a] = __builtin_bit_cast(f16x8, s_a[st][u][1][2 * wm + a][lane]);
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        bh[t] = __builtin_bit_cast(f16x8, s_b[st][u][0][2 * wn + t][lane]);
        bl[t] = __builtin_bit_cast(f16x8, s_b[st][u][1][2 * wn + t][lane]);
      }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[a], bh[t], acc[a][t], 0, 0, 0);
          acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[a], bl[t], acc[a][t], 0, 0, 0);
          acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[a], bh[t], acc[a][t], 0, 0, 0);
        }
    }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int c = n0 + 64 * wn + 32 * t + j;
    if (c >= n) continue;
    const float bias = bz ? bz[c] : 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = p0 + 64 * wm + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (row < hw) {
          if constexpr (OUT16) ((_Float16*)out)[((size_t)b * hw + row) * n + c] = (_Float16)(acc[a][t][r] + bias);
          else out[((size_t)b * hw + row) * n + c] = acc[a][t][r] + bias;
        }
      }
  }
}

// Exact-fp32 projection through LDS (round 5).  The form above fetches every operand of every MFMA straight from global memory
// (one 4-byte load per lane and matrix instruction): 0.27 ms per C2 map = 0.45 of the fp32-MFMA peak, replicated on every rank of a
// ray-sharded frame.  Here a workgroup owns a 128-texel x 128-channel tile, K is swept 16 at a time: every thread fetches 8 k-values
// of ONE texel (A) and of ONE channel (B) -- coalesced across the threads, the next step's loads in flight during this step's MFMAs
// -- and writes them to LDS as [k][128] lines (conflict-free both ways: a wave half reads 32 consecutive floats of one line); each
// of the four waves computes a 64 x 64 sub-tile from 4 LDS reads per 4 MFMAs.  Products and their order are the direct form's (every
// accumulator sees k = 0, 1, 2, ... through the same v_mfma_f32_32x32x2_f32 sequence): bit-identical output on six shapes
// (tools/diag/diag_project_ab.py).  Measured, one box: C2 map 0.275 -> 0.231 ms (0.53 of the peak), seven training images 1.60 ->
// 1.32 ms, 256 x 256 map 0.96 -> 0.80 ms; a 64-texel tile (twice the workgroups, six resident per CU) measured the same 0.235 ms,
// so the remaining gap to the fused kernels' 0.85 is not the tail of the launch -- per 2,048 cycles of MFMAs a wave also issues 16
// global loads, 16 LDS writes and a barrier, and its LDS reads are waited for one k-pair at a time.
__global__ void __launch_bounds__(256, 2) project_kernel_f32_lds(const float* __restrict__ feats, const float* __restrict__ wz,
                                                                const float* __restrict__ bz, int hw, int n, int ld, int K,
                                                                float* __restrict__ out) {
  constexpr int KS = 16;
  __shared__ float s_a[2][KS][128];
  __shared__ float s_b[2][KS][128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, kh = lane >> 5;
  const int b = blockIdx.z;
  const int p0 = blockIdx.x * 128, n0 = blockIdx.y * 128;
  const int lr = tid & 127, lk = tid >> 7;   // loader role: row lr of the tile, k-group lk (8 consecutive k of a step's 16)
  const float* fa = feats + (size_t)b * K * hw + min(p0 + lr, hw - 1);
  const float* fb = wz + min(n0 + lr, n - 1);
  const int wm = wave & 1, wn = wave >> 1;   // compute role: texel blocks 2*wm, 2*wm+1 x channel blocks 2*wn, 2*wn+1
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[a][t] = (f32x16)(0.f);
  float xa[8], xb[8];
  auto fetch = [&](int k0) {
    const int kb = k0 + 8 * lk;
#pragma unroll
    for (int i = 0; i < 8; ++i) xa[i] = fa[(size_t)(kb + i) * hw];
#pragma unroll
    for (int i = 0; i < 8; ++i) xb[i] = fb[(size_t)(kb + i) * ld];
  };
  fetch(0);
  int st = 0;
  for (int k0 = 0; k0 < K; k0 += KS, st ^= 1) {   // K is a multiple of 16 (checked by the launchers)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      s_a[st][8 * lk + i][lr] = xa[i];
      s_b[st][8 * lk + i][lr] = xb[i];
    }
    __syncthreads();  // stage `st` complete; every wave finished reading the other stage before it arrived here
    if (k0 + KS < K) fetch(k0 + KS);
#pragma unroll
    for (int kk = 0; kk < KS; kk += 2) {
      float av[2], bv[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) av[a] = s_a[st][kk + kh][64 * wm + 32 * a + j];
#pragma unroll
      for (int t = 0; t < 2; ++t) bv[t] = s_b[st][kk + kh][64 * wn + 32 * t + j];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int a = 0; a < 2; ++a) acc[a][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[t], acc[a][t], 0, 0, 0);
    }
  }
  // D layout: col = lane&31 (channel), row = (r&3) + 8*(r>>2) + 4*(lane>>5) (texel)
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int c = n0 + 64 * wn + 32 * t + j;
    if (c >= n) continue;
    const float bias = bz ? bz[c] : 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = p0 + 64 * wm + 32 * a + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (row < hw) out[((size_t)b * hw + row) * n + c] = acc[a][t][r] + bias;
      }
  }
}

static void launch_project(const float* feats, int K, const float* wz, int ld, const float* bz, int batch, int hw, int n,
                           float* out, int precision, hipStream_t s, bool out16 = false) {
  if (precision != NJF_PRECISION_F32) {  // F16X2, F16F6, F16: both operands split on the fly
    dim3 grid((hw + 127) / 128, (n + 127) / 128, batch);
    if (out16) project_kernel_f16x2<16, true><<<grid, 256, 0, s>>>(feats, wz, bz, hw, n, ld, K, out);
    else project_kernel_f16x2<16><<<grid, 256, 0, s>>>(feats, wz, bz, hw, n, ld, K, out);
  } else {
    dim3 grid((hw + 127) / 128, (n + 127) / 128, batch);
    project_kernel_f32_lds<<<grid, 256, 0, s>>>(feats, wz, bz, hw, n, ld, K, out);
  }
}

extern "C" int njf_project_features_ld(const float* feats, const float* wz, int wz_ld, const float* bz, int batch, int hw,
                                       int n, float* out, int precision, void* stream) {
  if (!feats || !wz || !bz || !out) return NJF_E_NULL;
  if (batch < 1 || hw < 1 || n < 1 || wz_ld < n) return NJF_E_SHAPE;
  if (!valid_base_precision(precision)) return NJF_E_MODE;
  // NJF_PRECISION_F16: `out` is a map of HALVES [batch, hw, n] (include/njf_hip.h)
  launch_project(feats, 512, wz, wz_ld, bz, batch, hw, n, out, precision, (hipStream_t)stream, precision == NJF_PRECISION_F16);
  return launch_status();
}

extern "C" int njf_project_features(const float* feats, const float* wz, const float* bz, int batch, int hw, int n,
                                    float* out, int precision, void* stream) {
  return njf_project_features_ld(feats, wz, n, bz, batch, hw, n, out, precision, stream);
}

// ---------------------------------------------------------------------------------------------
// Feature-pyramid producer (encoder_resnet.py:78-86 + the lin_z hoist): the encoder's output is
// cat_l(upsample_l(latent_l)); projection and bilinear up-sampling are both linear and act on different axes, so
// G = bz + sum_l upsample_l(latent_l . Wz[rows of level l]).  Each level is projected at its OWN resolution
// (5.6x fewer FLOPs than projecting the concatenated map, which is never formed), level 0 straight into `out`;
// this kernel then adds the up-sampled coarser levels in place.  One thread = 4 channels of one texel.
// ---------------------------------------------------------------------------------------------
struct UpsampleArgs {
  const float* src[3];
  int h[3], w[3];
  int levels;
  int batch, height, width, n;
  float* out;
};

__global__ void __launch_bounds__(256) upsample_add_kernel(UpsampleArgs a) {
  const int n4 = a.n >> 2;
  const long long total = (long long)a.batch * a.height * a.width * n4;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % n4) * 4;
  const long long t = i / n4;
  const int x = (int)(t % a.width), y = (int)((t / a.width) % a.height), b = (int)(t / ((long long)a.width * a.height));
  f32x4 acc = *(const f32x4*)(a.out + ((size_t)t * a.n + c));
  for (int l = 0; l < a.levels; ++l) {
    // F.interpolate(mode="bilinear", align_corners=False): src = (dst + 0.5) * in / out - 0.5, clamped at 0
    const int h = a.h[l], w = a.w[l];
    const float sy = fmaxf(((float)y + 0.5f) * ((float)h / (float)a.height) - 0.5f, 0.f);
    const float sx = fmaxf(((float)x + 0.5f) * ((float)w / (float)a.width) - 0.5f, 0.f);
    const int y0 = min((int)sy, h - 1), x0 = min((int)sx, w - 1);
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const float wy = sy - (float)y0, wx = sx - (float)x0;
    const float* base = a.src[l] + (size_t)b * h * w * a.n + c;
    const f32x4 v00 = *(const f32x4*)(base + ((size_t)y0 * w + x0) * a.n), v01 = *(const f32x4*)(base + ((size_t)y0 * w + x1) * a.n);
    const f32x4 v10 = *(const f32x4*)(base + ((size_t)y1 * w + x0) * a.n), v11 = *(const f32x4*)(base + ((size_t)y1 * w + x1) * a.n);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float top = v00[e] * (1.0f - wx) + v01[e] * wx, bot = v10[e] * (1.0f - wx) + v11[e] * wx;
      acc[e] += top * (1.0f - wy) + bot * wy;
    }
  }
  *(f32x4*)(a.out + ((size_t)t * a.n + c)) = acc;
}

// The same sum for pyramids whose coarser levels are exact 2^-s images of level 0 (ResNet latents of an image whose sides
// divide by 32: every shape the reference trains and renders): one thread = 4 channels of a 4 x 4 block of texels.  The
// bilinear taps of a block are a 4 x 4 (s = 1), 3 x 3 (s = 2) or 2 x 2 (s >= 3) patch of the coarser level, loaded once
// into registers -- 29 tap reads per 16 texels instead of 192, which is what bound the per-texel form (13 of its 14
// 16-byte accesses per texel were taps served by L2).  Weights and the order of every sum are the per-texel form's
// (src = (dst + 0.5) / 2^s - 0.5 is exact in fp32, so floor(src) is the compile-time offset table below; clamped patch
// indices reproduce the border taps, whose weight is exactly 0 where the clamp changes the tap): bit-identical output.
template <int S>  // 1, 2, or 3 = "3 or more"
__device__ __forceinline__ void upsample_block_level(const float* __restrict__ src, int h, int w, int n, int shift, int bx, int by,
                                                     int height, int width, f32x4 (&acc)[4][4]) {
  constexpr int NC = S == 1 ? 4 : S == 2 ? 3 : 2;
  constexpr int OFF[4] = {0, S == 1 ? 1 : 0, S == 3 ? 0 : 1, S == 1 ? 2 : S == 2 ? 1 : 0};
  // floor((4 k + 0.5) / 2^s - 0.5) = (8 k + 1 - 2^s) >> (s + 1), arithmetic shift
  const int base_x = (8 * bx + 1 - (1 << shift)) >> (shift + 1), base_y = (8 * by + 1 - (1 << shift)) >> (shift + 1);
  f32x4 patch[NC][NC];
#pragma unroll
  for (int r = 0; r < NC; ++r) {
    const int yy = min(max(base_y + r, 0), h - 1);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int xx = min(max(base_x + c, 0), w - 1);
      patch[r][c] = *(const f32x4*)(src + ((size_t)yy * w + xx) * n);
    }
  }
  float wx[4], wy[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float sx = fmaxf(((float)(4 * bx + j) + 0.5f) * ((float)w / (float)width) - 0.5f, 0.f);
    const float sy = fmaxf(((float)(4 * by + j) + 0.5f) * ((float)h / (float)height) - 0.5f, 0.f);
    wx[j] = sx - (float)min((int)sx, w - 1);
    wy[j] = sy - (float)min((int)sy, h - 1);
  }
#pragma unroll
  for (int jy = 0; jy < 4; ++jy)
#pragma unroll
    for (int jx = 0; jx < 4; ++jx) {
      const f32x4 v00 = patch[OFF[jy]][OFF[jx]], v01 = patch[OFF[jy]][OFF[jx] + 1];
      const f32x4 v10 = patch[OFF[jy] + 1][OFF[jx]], v11 = patch[OFF[jy] + 1][OFF[jx] + 1];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float top = v00[e] * (1.0f - wx[jx]) + v01[e] * wx[jx], bot = v10[e] * (1.0f - wx[jx]) + v11[e] * wx[jx];
        acc[jy][jx][e] += top * (1.0f - wy[jy]) + bot * wy[jy];
      }
    }
}

struct UpsampleBlockArgs {
  UpsampleArgs u;
  int shift[3];
};

__global__ void __launch_bounds__(256) upsample_add_block_kernel(UpsampleBlockArgs p) {
  const UpsampleArgs& a = p.u;
  const int n4 = a.n >> 2, bw = a.width >> 2, bh = a.height >> 2;
  const long long total = (long long)a.batch * bh * bw * n4;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % n4) * 4;
  const long long t = i / n4;
  const int bx = (int)(t % bw), by = (int)((t / bw) % bh), b = (int)(t / ((long long)bw * bh));
  float* out = a.out + (((size_t)b * a.height + 4 * by) * a.width + 4 * bx) * a.n + c;
  f32x4 acc[4][4];
#pragma unroll
  for (int jy = 0; jy < 4; ++jy)
#pragma unroll
    for (int jx = 0; jx < 4; ++jx) acc[jy][jx] = *(const f32x4*)(out + ((size_t)jy * a.width + jx) * a.n);
  for (int l = 0; l < a.levels; ++l) {
    const float* src = a.src[l] + (size_t)b * a.h[l] * a.w[l] * a.n + c;
    if (p.shift[l] == 1) upsample_block_level<1>(src, a.h[l], a.w[l], a.n, 1, bx, by, a.height, a.width, acc);
    else if (p.shift[l] == 2) upsample_block_level<2>(src, a.h[l], a.w[l], a.n, 2, bx, by, a.height, a.width, acc);
    else upsample_block_level<3>(src, a.h[l], a.w[l], a.n, p.shift[l], bx, by, a.height, a.width, acc);
  }
#pragma unroll
  for (int jy = 0; jy < 4; ++jy)
#pragma unroll
    for (int jx = 0; jx < 4; ++jx) *(f32x4*)(out + ((size_t)jy * a.width + jx) * a.n) = acc[jy][jx];
}

// fp32 map -> fp16 map (the pyramid route of the plain-fp16 mode: the levels are summed in fp32 and rounded once)
__global__ void __launch_bounds__(256) map_to_f16_kernel(const float* __restrict__ src, long long quads, _Float16* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= quads) return;
  const f32x4 v = *(const f32x4*)(src + 4 * i);
  typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
  const f16x4 o = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
  *(f16x4*)(dst + 4 * i) = o;
}

// shift s with (h << s, w << s) == (height, width), or 0 if the level is not an exact 2^-s image
static int pyramid_shift(int h, int w, int height, int width) {
  for (int s = 1; s < 16; ++s)
    if ((long long)h << s == height && (long long)w << s == width) return s;
  return 0;
}

extern "C" int njf_project_pyramid(const NjfPyramidLevel* levels, int num_levels, const float* wz, int wz_ld, const float* bz,
                                   int batch, int n, float* out, float* workspace, int precision, void* stream) {
  if (!levels || !wz || !bz || !out) return NJF_E_NULL;
  if (num_levels < 1 || num_levels > 4 || batch < 1 || n < 4 || (n & 3) || wz_ld < n) return NJF_E_SHAPE;
  if (!valid_base_precision(precision)) return NJF_E_MODE;
  if (num_levels > 1 && !workspace) return NJF_E_NULL;
  int rows = 0;
  for (int l = 0; l < num_levels; ++l) {
    if (!levels[l].feats) return NJF_E_NULL;
    if (levels[l].channels < 16 || (levels[l].channels & 15) || levels[l].height < 1 || levels[l].width < 1) return NJF_E_SHAPE;
    rows += levels[l].channels;
  }
  if (rows != 512) return NJF_E_SHAPE;  // rows of wz = channels of the concatenated encoder output
  hipStream_t s = (hipStream_t)stream;
  UpsampleArgs u;
  u.levels = num_levels - 1;
  u.batch = batch;
  u.height = levels[0].height;
  u.width = levels[0].width;
  u.n = n;
  u.out = out;
  int row0 = 0;
  float* ws = workspace;
  // plain-fp16 map: one level is projected straight into the map of halves; a pyramid is summed in fp32 in the FIRST
  // batch * H0 * W0 * n floats of the workspace (which the caller sizes accordingly, include/njf_hip.h) and rounded once
  const bool f16map = precision == NJF_PRECISION_F16;
  float* level0 = out;
  if (f16map && num_levels > 1) {
    level0 = ws;
    ws += (size_t)batch * u.height * u.width * n;
    u.out = level0;
  }
  for (int l = 0; l < num_levels; ++l) {
    const int hw = levels[l].height * levels[l].width;
    float* dst = l == 0 ? level0 : ws;
    launch_project(levels[l].feats, levels[l].channels, wz + (size_t)row0 * wz_ld, wz_ld, l == 0 ? bz : nullptr, batch, hw, n,
                   dst, precision, s, f16map && num_levels == 1);
    if (l > 0) {
      u.src[l - 1] = ws;
      u.h[l - 1] = levels[l].height;
      u.w[l - 1] = levels[l].width;
      ws += (size_t)batch * hw * n;
    }
    row0 += levels[l].channels;
  }
  if (u.levels > 0) {
    UpsampleBlockArgs blk;
    blk.u = u;
    bool blocked = (u.height & 3) == 0 && (u.width & 3) == 0;
    for (int l = 0; l < u.levels; ++l) {
      blk.shift[l] = pyramid_shift(u.h[l], u.w[l], u.height, u.width);
      blocked = blocked && blk.shift[l] > 0;
    }
    if (blocked) {
      const long long total = (long long)batch * (u.height >> 2) * (u.width >> 2) * (n >> 2);
      upsample_add_block_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(blk);
    } else {
      const long long total = (long long)batch * u.height * u.width * (n >> 2);
      upsample_add_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(u);
    }
    if (f16map) {
      const long long quads = (long long)batch * u.height * u.width * (n >> 2);
      map_to_f16_kernel<<<(unsigned)((quads + 255) / 256), 256, 0, s>>>(level0, quads, (_Float16*)out);
    }
  }
  return launch_status();
}

// ---------------------------------------------------------------------------------------------
// The encoder's output itself, channels-last: out[t][:] = cat_l(upsample_l(latent_l))[t] (encoder_resnet.py:78-86:
// F.interpolate(bilinear, align_corners=False) to the level-0 resolution + torch.cat) as ONE pass from the NCHW latents
// into the [B*H0*W0, 512] matrix the lin_z weight-gradient GEMM contracts against (training backward; the forward pass
// never needs it -- njf_project_pyramid).  One thread = 4 channels of one texel; the latents are small and stay in L2,
// the 512-channel rows are written once, coalesced.
// ---------------------------------------------------------------------------------------------
struct ConcatArgs {
  const float* src[4];
  int c[4], h[4], w[4];
  int c0[5];  // first output channel of each level (+ total)
  int levels, batch;
  float* out;
};

// One workgroup = 64 texels of one row x 64 output channels.  Pass 1: lane = texel, wave = 16 of the channels, so the
// four bilinear taps of every NCHW plane are read along x (coalesced); the tile is transposed through LDS (row pitch 65:
// conflict-free both ways).  Pass 2: 16 consecutive threads write the 64 channels of one texel as 256 contiguous bytes.
// (The round-1 form read the planes channel-major per thread: 16 scattered 4-byte loads per thread, 0.49 ms for the
// 235 MB matrix of the training batch; this form is bound by the write.)
__global__ void __launch_bounds__(256) upsample_concat_kernel(ConcatArgs a) {
  __shared__ float tile[64 * 65];
  const int n = a.c0[a.levels];
  const int height = a.h[0], width = a.w[0];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int groups = (n + 63) >> 6;
  const int xt = blockIdx.x / groups, cg = blockIdx.x - xt * groups;
  const int y = blockIdx.y, b = blockIdx.z;
  const int x = min(xt * 64 + lane, width - 1);
  for (int g = 0; g < 4; ++g) {  // the wave's 16 channels in groups of 4 (a level holds a multiple of 4 channels)
    const int c = cg * 64 + 16 * wave + 4 * g;
    if (c >= n) break;
    int l = 0;
    while (l + 1 < a.levels && c >= a.c0[l + 1]) ++l;
    const int cl = c - a.c0[l], h = a.h[l], w = a.w[l];
    // F.interpolate(mode="bilinear", align_corners=False): src = (dst + 0.5) * in / out - 0.5, clamped at 0
    const float sy = fmaxf(((float)y + 0.5f) * ((float)h / (float)height) - 0.5f, 0.f);
    const float sx = fmaxf(((float)x + 0.5f) * ((float)w / (float)width) - 0.5f, 0.f);
    const int y0 = min((int)sy, h - 1), x0 = min((int)sx, w - 1);
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const float wy = sy - (float)y0, wx = sx - (float)x0;
    const size_t plane = (size_t)h * w;
    const float* base = a.src[l] + ((size_t)b * a.c[l] + cl) * plane;
    const int o00 = y0 * w + x0, o01 = y0 * w + x1, o10 = y1 * w + x0, o11 = y1 * w + x1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float* p = base + e * plane;
      const float top = p[o00] * (1.0f - wx) + p[o01] * wx;
      const float bot = p[o10] * (1.0f - wx) + p[o11] * wx;
      tile[lane * 65 + 16 * wave + 4 * g + e] = top * (1.0f - wy) + bot * wy;
    }
  }
  __syncthreads();
  const int q = threadIdx.x & 15, tr = threadIdx.x >> 4;
  const int cq = cg * 64 + 4 * q;
  if (cq >= n) return;
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int tx = 16 * pass + tr, gx = xt * 64 + tx;
    if (gx >= width) continue;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = tile[tx * 65 + 4 * q + e];
    *(f32x4*)(a.out + (((size_t)b * height + y) * width + gx) * n + cq) = o;
  }
}

extern "C" int njf_upsample_concat(const NjfPyramidLevel* levels, int num_levels, int batch, float* out, void* stream) {
  if (!levels || !out) return NJF_E_NULL;
  if (num_levels < 1 || num_levels > 4 || batch < 1) return NJF_E_SHAPE;
  ConcatArgs a;
  a.levels = num_levels;
  a.batch = batch;
  a.out = out;
  a.c0[0] = 0;
  for (int l = 0; l < num_levels; ++l) {
    if (!levels[l].feats) return NJF_E_NULL;
    if (levels[l].channels < 4 || (levels[l].channels & 3) || levels[l].height < 1 || levels[l].width < 1) return NJF_E_SHAPE;
    a.src[l] = levels[l].feats;
    a.c[l] = levels[l].channels;
    a.h[l] = levels[l].height;
    a.w[l] = levels[l].width;
    a.c0[l + 1] = a.c0[l] + levels[l].channels;
  }
  const long long tiles = (long long)((a.w[0] + 63) / 64) * ((a.c0[num_levels] + 63) / 64);
  if (tiles > 0x7fffffffLL || a.h[0] > 65535 || batch > 65535) return NJF_E_SHAPE;
  upsample_concat_kernel<<<dim3((unsigned)tiles, a.h[0], batch), 256, 0, (hipStream_t)stream>>>(a);
  return launch_status();
}

// ---------------------------------------------------------------------------------------------
// Adjoint of njf_upsample_concat for ONE level (the encoder tail's backward pass, encoder_resnet.py:78-86 differentiated:
// what autograd runs as slice + upsample_bilinear2d_backward per latent): grad [B*H0*W0, n] channels-last -> the gradient
// of the level's NCHW latent [B, C, h, w], channels c0 .. c0+C-1 of grad.  Gather form (no atomics, fixed summation
// order: bit-reproducible): a latent texel collects w_y * w_x * grad over the fine texels whose bilinear footprint
// contains it; the weights are recomputed with the forward pass's own formulas, so the kernel is the exact transpose of
// upsample_concat_kernel for any size ratio (the window is the support widened by one texel; weights outside are zero).
// One workgroup = 64 latent texels of one row x 64 channels: 16 lanes read 256 contiguous bytes of a fine texel's row,
// the tile is transposed through LDS and written along x (NCHW).
// ---------------------------------------------------------------------------------------------
struct ConcatBwdArgs {
  const float* grad;
  int n, H, W;     // fine map: channels, height, width
  int c0, C, h, w; // the level: first channel in grad, channels, height, width
  float* dst;      // [B, C, h, w]
};

__device__ __forceinline__ float bilinear_tap_weight(int fine, int coarse, int n_coarse, float ratio) {
  // weight of latent index `coarse` in the bilinear interpolation of fine index `fine` (align_corners=False)
  const float s = fmaxf(((float)fine + 0.5f) * ratio - 0.5f, 0.f);
  const int i0 = min((int)s, n_coarse - 1), i1 = min(i0 + 1, n_coarse - 1);
  const float t = s - (float)i0;
  return (i0 == coarse ? 1.0f - t : 0.f) + (i1 == coarse ? t : 0.f);
}

__global__ void __launch_bounds__(256) upsample_concat_backward_kernel(ConcatBwdArgs a) {
  __shared__ float tile[64 * 65];
  const int groups = (a.C + 63) >> 6;
  const int xt = blockIdx.x / groups, cg = blockIdx.x - xt * groups;
  const int yc = blockIdx.y, b = blockIdx.z;
  const int q = threadIdx.x & 15, tr = threadIdx.x >> 4;
  const int c = cg * 64 + 4 * q;
  const float ry = (float)a.h / (float)a.H, rx = (float)a.w / (float)a.W;
  const int y_lo = max(0, (int)floorf(((float)yc - 0.5f) / ry - 0.5f) - 1);
  const int y_hi = min(a.H - 1, (int)ceilf(((float)yc + 1.5f) / ry - 0.5f) + 1);
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int tx = 16 * pass + tr, xc = xt * 64 + tx;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (xc < a.w && c < a.C) {
      const int x_lo = max(0, (int)floorf(((float)xc - 0.5f) / rx - 0.5f) - 1);
      const int x_hi = min(a.W - 1, (int)ceilf(((float)xc + 1.5f) / rx - 0.5f) + 1);
      for (int y = y_lo; y <= y_hi; ++y) {
        const float wy = bilinear_tap_weight(y, yc, a.h, ry);
        if (wy == 0.f) continue;
        const float* row = a.grad + (((size_t)b * a.H + y) * a.W) * a.n + a.c0 + c;
        for (int x = x_lo; x <= x_hi; ++x) {
          const float wx = bilinear_tap_weight(x, xc, a.w, rx);
          if (wx == 0.f) continue;
          const f32x4 g = *(const f32x4*)(row + (size_t)x * a.n);
          const float wgt = wy * wx;
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = fmaf(wgt, g[e], acc[e]);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) tile[tx * 65 + 4 * q + e] = acc[e];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = xt * 64 + lane;
  if (x >= a.w) return;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int ch = cg * 64 + 16 * wave + g;
    if (ch < a.C) a.dst[(((size_t)b * a.C + ch) * a.h + yc) * a.w + x] = tile[lane * 65 + 16 * wave + g];
  }
}

extern "C" int njf_upsample_concat_backward(const float* grad, const NjfPyramidLevel* levels, int num_levels, int batch,
                                            void* stream) {
  if (!grad || !levels) return NJF_E_NULL;
  if (num_levels < 1 || num_levels > 4 || batch < 1 || batch > 65535) return NJF_E_SHAPE;
  int n = 0;
  for (int l = 0; l < num_levels; ++l) {
    if (!levels[l].feats) return NJF_E_NULL;
    if (levels[l].channels < 4 || (levels[l].channels & 3) || levels[l].height < 1 || levels[l].width < 1 ||
        levels[l].height > 65535)
      return NJF_E_SHAPE;
    n += levels[l].channels;
  }
  int c0 = 0;
  for (int l = 0; l < num_levels; ++l) {
    ConcatBwdArgs a{grad, n, levels[0].height, levels[0].width, c0, levels[l].channels, levels[l].height, levels[l].width,
                    const_cast<float*>(levels[l].feats)};  // the record's pointer is the OUTPUT of this entry point
    const long long tiles = (long long)((a.w + 63) / 64) * ((a.C + 63) / 64);
    if (tiles > 0x7fffffffLL) return NJF_E_SHAPE;
    upsample_concat_backward_kernel<<<dim3((unsigned)tiles, a.h, batch), 256, 0, (hipStream_t)stream>>>(a);
    c0 += levels[l].channels;
  }
  return launch_status();
}

// =============================================================================================
// batched 4x4 inverse (camera matrices: torch.inverse in rendering/geometry.py:52,64)
// =============================================================================================
// One thread per matrix: Gauss-Jordan elimination with partial pivoting on [M | I] in registers (fp64).  Replaces the
// LAPACK-style getrf/getri sequence torch.linalg.inv launches per call (6 kernels + workspace fills, ~40 us of launch
// latency for a 64-byte problem; three such calls per forward pass were a quarter of a 8,192-ray step).
__global__ void invert4x4_kernel(const float* __restrict__ m, int n, float* __restrict__ out) {
  // Evaluated in float64 and rounded once: the result is the correctly rounded inverse (to ~0.5 ulp), so it differs
  // from the reference's fp32 LAPACK inverse only by LAPACK's own rounding error.  That matters: the context pose's
  // inverse feeds the positional encoding (2*pi*512 gain), where one ulp of a matrix entry is ~1e-4 of the outputs --
  // an fp32 Gauss-Jordan (2-3 ulp off) measured 4e-4 on the optical flow of a general-pose fixture, this form 7e-5.
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double a[4][8];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      a[r][c] = (double)m[i * 16 + r * 4 + c];
      a[r][4 + c] = r == c ? 1.0 : 0.0;
    }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    int p = c;
    double best = fabs(a[c][c]);
#pragma unroll
    for (int r = c + 1; r < 4; ++r) {
      const double v = fabs(a[r][c]);
      if (v > best) {
        best = v;
        p = r;
      }
    }
#pragma unroll
    for (int r = c + 1; r < 4; ++r)  // swap rows c and p (static indices: the arrays stay in registers)
      if (p == r) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const double t = a[c][k];
          a[c][k] = a[r][k];
          a[r][k] = t;
        }
      }
    const double inv = 1.0 / a[c][c];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[c][k] *= inv;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (r == c) continue;
      const double f = a[r][c];
#pragma unroll
      for (int k = 0; k < 8; ++k) a[r][k] = fma(-f, a[c][k], a[r][k]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) out[i * 16 + r * 4 + c] = (float)a[r][4 + c];
}

extern "C" int njf_invert_4x4(const float* matrices, int count, float* out, void* stream) {
  if (!matrices || !out) return NJF_E_NULL;
  if (count < 1) return NJF_E_SHAPE;
  invert4x4_kernel<<<(count + 63) / 64, 64, 0, (hipStream_t)stream>>>(matrices, count, out);
  return launch_status();
}

// =============================================================================================
// ray generation (rendering/geometry.py:117-134, :170-203)
// =============================================================================================
__global__ void raygen_kernel(const float* __restrict__ coords, int height, int width, const float* __restrict__ k_inv,
                              const float* __restrict__ c2w, int batch, int rays, float* __restrict__ origins,
                              float* __restrict__ directions, float* __restrict__ z) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch * rays) return;
  const int b = i / rays, r = i - b * rays;
  float x, y;
  if (coords) {
    x = coords[2 * (size_t)i];
    y = coords[2 * (size_t)i + 1];
  } else {  // get_pixel_coordinates: x = (col + 0.5) / W, y = (row + 0.5) / H, row-major pixels
    const int row = r / width, col = r - row * width;
    x = ((float)col + 0.5f) / (float)width;
    y = ((float)row + 0.5f) / (float)height;
  }
  const float* ki = k_inv + b * 9;
  // einsum("cij,crj->cri", K^-1, [x, y, 1]): fma chain in j order (see point_geometry)
  float cx = fmaf(ki[2], 1.0f, fmaf(ki[1], y, ki[0] * x));
  float cy = fmaf(ki[5], 1.0f, fmaf(ki[4], y, ki[3] * x));
  float cz = fmaf(ki[8], 1.0f, fmaf(ki[7], y, ki[6] * x));
  cx *= 1.0f;  // unproject multiplies by z = 1 (geometry.py:56)
  const float nrm = sqrtf(cx * cx + cy * cy + cz * cz);
  cx /= nrm;
  cy /= nrm;
  cz /= nrm;
  const float* m = c2w + b * 16;
  const float dx = fmaf(m[3], 0.0f, fmaf(m[2], cz, fmaf(m[1], cy, m[0] * cx)));
  const float dy = fmaf(m[7], 0.0f, fmaf(m[6], cz, fmaf(m[5], cy, m[4] * cx)));
  const float dz = fmaf(m[11], 0.0f, fmaf(m[10], cz, fmaf(m[9], cy, m[8] * cx)));
  origins[3 * (size_t)i + 0] = m[3];
  origins[3 * (size_t)i + 1] = m[7];
  origins[3 * (size_t)i + 2] = m[11];
  directions[3 * (size_t)i + 0] = dx;
  directions[3 * (size_t)i + 1] = dy;
  directions[3 * (size_t)i + 2] = dz;
  if (z) z[i] = cz;
}

extern "C" int njf_generate_rays(const float* coords, int height, int width, const float* k_inv, const float* c2w,
                                 int batch, int rays, float* origins, float* directions, float* z, void* stream) {
  if (!k_inv || !c2w || !origins || !directions) return NJF_E_NULL;
  if (batch < 1 || rays < 1) return NJF_E_SHAPE;
  if (!coords && (height < 1 || width < 1 || (long long)height * width != rays)) return NJF_E_SHAPE;
  const int n = batch * rays;
  raygen_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(coords, height, width, k_inv, c2w, batch, rays, origins,
                                                                 directions, z);
  return launch_status();
}

// ---- a depth frame to world points (njf_field_depth_points) -------------------------------------------------
// One lane per pixel: the validity of its depth and of its four neighbours, raygen_kernel's ray of the pixel centre -- the same
// expressions in the same order, restated here so that raygen_kernel is not touched --, t from the depth, and the point o + d t
// as one multiply and one add per component.  Every row is written; `kept` is counted with integer atomics.
struct DepthArgs {
  const float* depth;  // [B,H,W]
  const float* k_inv;  // [B,3,3]
  const float* c2w;    // [B,4,4]
  int batch, height, width, views;
  long long rays;      // H * W
  long long total;     // B * H * W < 2^31
  int kind;
  float near, far, max_jump;
  float* points;       // [B,H*W,3]
  int* kept;           // [B / views]
};

__device__ __forceinline__ bool depth_valid(float d, float near, float far) {
  return fabsf(d) < INFINITY && d > near && d <= far;  // (NaN compares false)
}

// a valid neighbour across a depth edge: the rule is symmetric in (d, dn)
__device__ __forceinline__ bool depth_jump(float d, float dn, const DepthArgs& a) {
  return depth_valid(dn, a.near, a.far) && fabsf(d - dn) > a.max_jump * fminf(d, dn);
}

__global__ void __launch_bounds__(256) depth_points_kernel(DepthArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < a.total;
  const int b = live ? (int)(i / a.rays) : 0;
  const int scene = live ? b / a.views : -1;
  bool ok = false;
  if (live) {
    const int r = (int)(i - (long long)b * a.rays);
    const int row = r / a.width, col = r - row * a.width;
    const float* img = a.depth + (long long)b * a.rays;
    const float d = img[r];
    ok = depth_valid(d, a.near, a.far);
    if (ok && a.max_jump > 0.0f) {
      if (row > 0 && depth_jump(d, img[r - a.width], a)) ok = false;
      if (row + 1 < a.height && depth_jump(d, img[r + a.width], a)) ok = false;
      if (col > 0 && depth_jump(d, img[r - 1], a)) ok = false;
      if (col + 1 < a.width && depth_jump(d, img[r + 1], a)) ok = false;
    }
    float px = __int_as_float(0x7fc00000), py = px, pz = px;
    if (ok) {
      const float x = ((float)col + 0.5f) / (float)a.width;
      const float y = ((float)row + 0.5f) / (float)a.height;
      const float* ki = a.k_inv + b * 9;
      float cx = fmaf(ki[2], 1.0f, fmaf(ki[1], y, ki[0] * x));
      float cy = fmaf(ki[5], 1.0f, fmaf(ki[4], y, ki[3] * x));
      float cz = fmaf(ki[8], 1.0f, fmaf(ki[7], y, ki[6] * x));
      cx *= 1.0f;
      const float nrm = sqrtf(cx * cx + cy * cy + cz * cz);
      cx /= nrm;
      cy /= nrm;
      cz /= nrm;
      const float* m = a.c2w + b * 16;
      const float dx = fmaf(m[3], 0.0f, fmaf(m[2], cz, fmaf(m[1], cy, m[0] * cx)));
      const float dy = fmaf(m[7], 0.0f, fmaf(m[6], cz, fmaf(m[5], cy, m[4] * cx)));
      const float dz = fmaf(m[11], 0.0f, fmaf(m[10], cz, fmaf(m[9], cy, m[8] * cx)));
      const float t = a.kind == NJF_FIELD_DEPTH_Z ? d / cz : d;
      px = m[3] + dx * t;
      py = m[7] + dy * t;
      pz = m[11] + dz * t;
    }
    a.points[3 * i + 0] = px;
    a.points[3 * i + 1] = py;
    a.points[3 * i + 2] = pz;
  }
  // one atomic per wave where its pixels belong to one scene (lane 0 is live whenever any lane is)
  const int first = __shfl(scene, 0, 64);
  if (__all(!ok || scene == first)) {
    const int n = __popcll(__ballot(ok));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&a.kept[first], n);
  } else if (ok) {
    atomicAdd(&a.kept[scene], 1);
  }
}

extern "C" int njf_field_depth_points(const float* depth, int batch, int height, int width, const float* k_inv, const float* c2w,
                                      int kind, float near, float far, float max_jump, int views_per_scene, float* points,
                                      int* kept, void* stream) {
  if (!depth || !k_inv || !c2w || !points || !kept) return NJF_E_NULL;
  if (batch < 1 || height < 1 || width < 1 || (long long)batch * height * width >= (1LL << 31)) return NJF_E_SHAPE;
  if (views_per_scene < 1 || batch % views_per_scene) return NJF_E_SHAPE;
  if (kind != NJF_FIELD_DEPTH_RAY && kind != NJF_FIELD_DEPTH_Z) return NJF_E_VALUE;
  if (!(near >= 0.0f) || !(near < INFINITY) || !(far > near)) return NJF_E_VALUE;
  if (!(max_jump >= 0.0f) || !(max_jump < INFINITY)) return NJF_E_VALUE;
  DepthArgs a;
  a.depth = depth;
  a.k_inv = k_inv;
  a.c2w = c2w;
  a.batch = batch;
  a.height = height;
  a.width = width;
  a.views = views_per_scene;
  a.rays = (long long)height * width;
  a.total = a.rays * batch;
  a.kind = kind;
  a.near = near;
  a.far = far;
  a.max_jump = max_jump;
  a.points = points;
  a.kept = kept;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(kept, 0, (size_t)(batch / views_per_scene) * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  depth_points_kernel<<<(unsigned)((a.total + 255) / 256), 256, 0, s>>>(a);
  return launch_status();
}

// =============================================================================================
// shared pieces of the fused ray kernels
// =============================================================================================
// chunks of a ResnetFC a kernel streams per tile: the plain-fp16 form holds a whole 128 x 128 layer per chunk
template <int PREC>
constexpr int resnet_chunks() { return PREC == PREC_F16 ? NJF_RESNET_CHUNKS_F16 : NJF_RESNET_CHUNKS; }
// ... and where the stream skips the unused slots of the FIRST network's blob (WeightStreamT<GAP_AT, GAP>; the blobs keep
// their NJF_RESNET_CHUNKS-slot extent in every precision)
template <int PREC>
constexpr int resnet_gap_at() { return PREC == PREC_F16 ? NJF_RESNET_CHUNKS_F16 : 0x7fffffff; }
template <int PREC>
constexpr int resnet_gap() { return PREC == PREC_F16 ? NJF_RESNET_CHUNKS - NJF_RESNET_CHUNKS_F16 : 0; }

struct RayCommon {
  const float* origins;
  const float* directions;
  int rays_per_batch;
  int total_rays;
  NjfCameras cams;
  NjfFeatureMap gmap;
};

__device__ __forceinline__ void load_bias_block(const float* __restrict__ src, int n, int dst_off) {
  for (int i = threadIdx.x; i < n; i += NJF_THREADS) njf_lds[LDS_BIAS + dst_off + i] = src[i];
}

// alpha = 1 - exp(-ds), ds >= 0 (ray_samplers.py:93-95), WITHOUT the cancellation of the literal form.  In fp32
// `1 - exp(-ds)` is a multiple of 2^-24 whatever its size, so a sample in nearly empty space (ds ~ 1e-6) carries its weight
// with 5-25 % relative error -- in the reference too -- and two correct exp implementations (device libm here, Sleef in
// torch's CPU path) that round exp(-ds) to different neighbours disagree by a whole quantum.  Harmless for the composited
// pixels (sums dominated by large weights), but the ds-nerf depth loss differentiates log(w + 1e-7) (utils/loss_utils.py:
// 9-35): its upstream gradient 1 / (w + 1e-7) is LARGEST exactly on those weights, and the one-quantum disagreement was the
// 2.3-2.9e-3 deviation of every proposal-net gradient from the oracle (tools/diag/diag_perception.py, round 4; same in exact
// fp32 and split precision).  Evaluated accurately -- Taylor to x^5 below 2^-4 (truncation 1.3e-9 relative), the literal form
// above it (relative error <= 1e-6) -- the weights follow the float64 result instead of a rounding accident, and the
// gradients fall inside twice the oracle's own fp32-vs-float64 floors.
__device__ __forceinline__ float alpha_of(float ds) {
  const float series = ds * fmaf(-0.5f * ds, fmaf(-(1.0f / 3.0f) * ds, fmaf(-0.25f * ds, fmaf(-0.2f, ds, 1.0f), 1.0f), 1.0f), 1.0f);
  return ds < 0.0625f ? series : 1.0f - expf(-ds);
}

// alpha compositing weights of one 32-sample tile (ray_samplers.py:77-101), carrying the running
// optical depth across tiles.
__device__ __forceinline__ float tile_weights(float delta, float sigma, bool valid, int j, float& carry) {
  const float ds = (valid && delta > 0.f) ? delta * sigma : 0.f;
  const float incl = half_scan(ds, j);
  float excl = __shfl_up(incl, 1, 32);
  if (j == 0) excl = 0.f;
  excl += carry;
  carry += __shfl(incl, 31, 32);
  return alpha_of(ds) * expf(-excl);
}

// inverse-CDF resampling of one ray (ray_samplers.py:351-451).  w' (already annealed, +padding not
// yet applied) lives in sc[0..s_in); cdf is built in sc[256..256+s_in].  All 64 lanes cooperate.
__device__ __forceinline__ void pdf_resample_ray(float* __restrict__ sc, const float* __restrict__ bins_in, int s_in,
                                                 const float* __restrict__ u, int s_out, float* __restrict__ bins_out,
                                                 int lane, bool store) {
  float part = 0.f;
  for (int i = lane; i < s_in; i += 64) part += sc[i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o, 64);
  float wsum = part;
  const float pad = fmaxf(1e-5f - wsum, 0.f);
  const float padper = pad / (float)s_in;
  wsum += pad;
  // inclusive cumsum of pdf: contiguous run per lane + wave scan of run totals
  const int per = (s_in + 63) >> 6;
  const int i0 = lane * per;
  float run = 0.f;
  for (int i = 0; i < per; ++i) {
    const int s = i0 + i;
    if (s < s_in) run += (sc[s] + padper) / wsum;
  }
  float incl = run;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  float acc = incl - run;
  float* cdf = sc + 256;
  __syncthreads();  // all lanes have read sc[] for wsum before anyone overwrites (uniform control flow)
  for (int i = 0; i < per; ++i) {
    const int s = i0 + i;
    if (s < s_in) {
      acc += (sc[s] + padper) / wsum;
      cdf[s + 1] = fminf(1.0f, acc);
    }
  }
  if (lane == 0) cdf[0] = 0.f;
  __syncthreads();
  for (int k = lane; k <= s_out; k += 64) {
    const float uk = u[k];
    int lo = 0, hi = s_in + 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cdf[mid] <= uk) lo = mid + 1;
      else hi = mid;
    }
    const int below = min(max(lo - 1, 0), s_in), above = min(max(lo, 0), s_in);
    const float c0 = cdf[below], c1 = cdf[above];
    const float g0 = bins_in[below], g1 = bins_in[above];
    float t = (uk - c0) / (c1 - c0);
    if (t != t) t = 0.f;  // nan_to_num(nan=0); +-inf are absorbed by the clip
    t = fminf(fmaxf(t, 0.f), 1.f);
    if (store) bins_out[k] = g0 + t * (g1 - g0);
  }
}

// =============================================================================================
// proposal pass
// =============================================================================================
struct ProposalArgs {
  RayCommon rc;
  int gmap_offset;
  const float* w_pack;
  const float* b_pack;
  const float* bins_in;
  int bins_per_ray;
  int s_in;
  const float* u;
  int u_per_ray;
  int s_out;
  float anneal;
  float* bins_out;
  float* weights_out;
  float* density_out;
  NjfActivationDump dump;  // DUMP instantiation only (training forward)
};

// this lane's share of a point's backward-pass inputs: activations / encoding (both halves), footprint (half 0)
__device__ __forceinline__ ActDump point_dump(const NjfActivationDump& d, size_t pidx, size_t points, int hh,
                                              const PointGeom& g, int tex0, int texel_stride) {
  float* act = nullptr;   // this lane's 64 values of layer 0 (floats, or halves under the 16-bit training storage)
  if (d.act) act = d.act_f16 ? (float*)((_Float16*)d.act + pidx * 128 + 64 * hh) : d.act + pidx * 128 + 64 * hh;
  ActDump dump{act, d.pe + pidx * 64 + 32 * hh, points * 128, d.mask ? d.mask + pidx * 4 + 2 * hh : nullptr, d.act_f16 != 0};
  if (hh == 0 && d.foot_idx != nullptr) {
    Footprint f;
    point_footprint(g, f);
    int* fi = d.foot_idx + pidx * 4;
    fi[0] = tex0 + f.t00 / texel_stride;
    fi[1] = tex0 + f.t01 / texel_stride;
    fi[2] = tex0 + f.t10 / texel_stride;
    fi[3] = tex0 + f.t11 / texel_stride;
    float* fw = d.foot_w + pidx * 4;
    fw[0] = f.w00;
    fw[1] = f.w01;
    fw[2] = f.w10;
    fw[3] = f.w11;
  }
  return dump;
}

template <int PREC, bool DUMP = false>
__global__ void __launch_bounds__(NJF_THREADS, 2) proposal_kernel(ProposalArgs a) {
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, j = lane & 31, hh = lane >> 5;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int ray = wg * NJF_WAVES + wave;
  const bool ray_ok = ray < a.rc.total_rays;
  const int rayc = min(ray, a.rc.total_rays - 1);
  const int b = rayc / a.rc.rays_per_batch;

  load_bias_block(a.b_pack, NJF_RESNET_B_FLOATS, 0);
  const int tiles = (a.s_in + 31) >> 5;
  WeightStream st;
  stream_begin(st, a.w_pack, resnet_chunks<PREC>(), tiles, wave, lane);
  NJF_STAMP_ARM(st, true, wave);

  CamCtx cam;
  load_ctx(a.rc.cams.ctxt_w2c, a.rc.cams.ctxt_k, b, cam);
  const float near = a.rc.cams.z_near[b], far = a.rc.cams.z_far[b];
  const float ox = a.rc.origins[3 * (size_t)rayc], oy = a.rc.origins[3 * (size_t)rayc + 1],
              oz = a.rc.origins[3 * (size_t)rayc + 2];
  const float dx = a.rc.directions[3 * (size_t)rayc], dy = a.rc.directions[3 * (size_t)rayc + 1],
              dz = a.rc.directions[3 * (size_t)rayc + 2];
  const float* gz = map_at<PREC>(a.rc.gmap.data, (size_t)b * a.rc.gmap.height * a.rc.gmap.width * a.rc.gmap.stride + a.gmap_offset);
  const float* bins = a.bins_in + (a.bins_per_ray ? (size_t)rayc * (a.s_in + 1) : 0);
  float* sc = njf_lds + LDS_SCRATCH_PROPOSAL + wave * LDS_SCRATCH_PER_WAVE;
  const float* bias = njf_lds + LDS_BIAS;

  float carry = 0.f;
  for (int t = 0; t < tiles; ++t) {
    const int s = t * 32 + j;
    const bool valid = s < a.s_in;
    const int sc_i = min(s, a.s_in - 1);
    const float b0 = bins[sc_i], b1 = bins[sc_i + 1];
    const float start = b0 * far + (1.0f - b0) * near;
    const float end = b1 * far + (1.0f - b1) * near;
    const float se = start + end;
    const float px = ox + (dx * se) / 2.0f, py = oy + (dy * se) / 2.0f, pz = oz + (dz * se) / 2.0f;
    PointGeom g;
    point_geometry(cam, px, py, pz, a.rc.gmap.height, a.rc.gmap.width, a.rc.gmap.stride, 0u, g);
    NJF_STAMP_P(st, 10);
    f32x16 pe[2];
    positional_encoding(g.xc, g.yc, g.zc, hh, pe);
    f32x16 out[1];
    ActDump dump{nullptr, nullptr, 0};
    if (DUMP && valid && ray_ok)
      dump = point_dump(a.dump, (size_t)ray * a.s_in + s, (size_t)a.rc.total_rays * a.s_in, hh, g,
                        b * a.rc.gmap.height * a.rc.gmap.width, a.rc.gmap.stride);
    // (plain fp16: one footprint for the three gathers + lin_in from a packed encoding, as in the render kernel, measured 0.7 %
    //  SLOWER here -- profiles/r05_ablate_f16.txt block k -- and is not used)
    resnet_tile<PREC, DUMP>(st, bias, gz, g, pe, wave, lane, out, dump);
    NJF_STAMP_P(st, 14);
    const float pre = __shfl(out[0][0], j, 64);
    const float sigma = expf(pre - 1.0f);
    const float w = tile_weights(end - start, sigma, valid, j, carry);
    if (valid && hh == 0) {
      float wa = w;
      if (a.anneal != 1.0f) wa = powf(w, a.anneal);
      sc[s] = wa + 0.01f;  // histogram_padding (ray_samplers.py:375)
      if (ray_ok) {
        if (a.weights_out) a.weights_out[(size_t)ray * a.s_in + s] = w;
        if (a.density_out) a.density_out[(size_t)ray * a.s_in + s] = sigma;
      }
    }
  }
  NJF_STAMP_P(st, 13);
  __syncthreads();
  const float* u = a.u + (a.u_per_ray ? (size_t)rayc * (a.s_out + 1) : 0);
  pdf_resample_ray(sc, bins, a.s_in, u, a.s_out, a.bins_out + (size_t)rayc * (a.s_out + 1), lane, ray_ok);
  NJF_STAMP_FLUSH(st, 15, lane);
}

// =============================================================================================
// decoder evaluation of one tile, stage by stage: density net -> colour head -> Jacobian head / flow.  The callers
// composite (or store) each stage's result before the next stage starts, so that only the sample weight, the
// camera-space position and the ray constants stay live across the 22 weight chunks of the Jacobian head.
// =============================================================================================
// bias layout (LDS_BIAS): [density 1312 | colour 96 | jacobian head (MLP 1312 / transformer 800)]
// JKIND: 0 = no Jacobian head, 1 = ResnetFC head (jacobian_mlp), 2 = folded transformer head (jacobian_transformer)
// DUMP: 0 = inference, 1 = dump the Jacobian ResnetFC (action-mode training), 2 = dump the density ResnetFC and the
// colour head (perception-mode training); `dump` addresses the dumped net, `cdump` the colour head.
// SHARE (plain-fp16 inference): the stage fills `share` (packed encoding + footprint of this tile's points, TileShareF16) for
// its own network and for a ResnetFC Jacobian head that follows.
template <int PREC, int DUMP, int SHARE = 0, class ST>
__device__ __forceinline__ float density_stage(ST& st, const float* __restrict__ gz_d, const PointGeom& g, int wave,
                                               int lane, f32x16 (&geo)[1], ActDump dump, TileShareF16* share = nullptr) {
  const int j = lane & 31, hh = lane >> 5;
  f32x16 pe[2];
  positional_encoding(g.xc, g.yc, g.zc, hh, pe);
  if constexpr (SHARE != 0) {
    share_tile(pe, *share);
    resnet_tile<PREC, false, SHARE>(st, njf_lds + LDS_BIAS, gz_d, g, pe, wave, lane, geo, dump, share);
  } else {
    resnet_tile<PREC, DUMP == 2>(st, njf_lds + LDS_BIAS, gz_d, g, pe, wave, lane, geo, dump);
  }
  return expf(__shfl(geo[0][15], j, 64) - 1.0f);
}

template <int PREC, int DUMP, class ST>
__device__ __forceinline__ void color_stage(ST& st, const f32x16 (&geo)[1], float dirx, float diry, float dirz,
                                            int wave, int lane, float (&rgb)[3], ColorDump cdump) {
  const int j = lane & 31, hh = lane >> 5;
  // The harmonics depend on the ray only, so the compiler computes them once in front of the tile loop -- and, with every
  // register taken by the networks, spills all 16 and reloads them here one by one behind s_waitcnt vmcnt(0) (which also
  // waits for the weight DMA in flight): 16 serialised memory round trips per tile for ~30 VALU instructions of work.
  // Opaque copies of the direction make it a per-tile recomputation.
  asm volatile("" : "+v"(dirx), "+v"(diry), "+v"(dirz));
  float sh[16];
  sh4(dirx, diry, dirz, sh);
  f32x16 cin[1], crgb[1];
#pragma unroll
  for (int r = 0; r < 16; ++r) cin[0][r] = hh ? sh[r] : (r < 15 ? geo[0][r] : 1.0f);
  color_tile<PREC, DUMP == 2>(st, njf_lds + LDS_BIAS + NJF_RESNET_B_FLOATS, cin, wave, lane, crgb, cdump);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float x = __shfl(crgb[0][c], j, 64);
    rgb[c] = 1.0f / (1.0f + expf(-x));
  }
}

template <int JKIND, int PREC, int DUMP, int SHARE = 0, class ST>
__device__ __forceinline__ void jacobian_stage(ST& st, const float* __restrict__ gz_j, const PointGeom& g,
                                               const float* __restrict__ action, int action_dim, int wave, int lane,
                                               f32x16 (&jac)[1], float (&flow)[3], ActDump dump, const TileShareF16* share = nullptr) {
  const int hh = lane >> 5;
  const float* bias = njf_lds + LDS_BIAS + NJF_RESNET_B_FLOATS + NJF_COLOR_B_FLOATS;
  if constexpr (SHARE != 0) {   // ResnetFC head in plain fp16: the density stage's packed encoding (TileShareF16)
    static_assert(JKIND == 1 && DUMP == 0, "shared tile state: ResnetFC Jacobian head, inference");
    NJF_STAMP(st, 6);
    NJF_STAMP(st, 7);
    f32x16 unused[2];
    resnet_tile<PREC, false, SHARE>(st, bias, gz_j, g, unused, wave, lane, jac, dump, share);
  } else {
  // the encoding is recomputed (~1 % of the head's time) rather than held in 32 VGPRs across density + colour
  // ... and REALLY recomputed: without the opaque copies the compiler keeps the density stage's 25 encoding values alive
  // through scratch and reloads them inside the lin_in chunk, each reload behind its own s_waitcnt vmcnt(0)
  float xc = g.xc, yc = g.yc, zc = g.zc;
  asm volatile("" : "+v"(xc), "+v"(yc), "+v"(zc) : : "memory");
  f32x16 pe[2];
  NJF_STAMP(st, 6);  // Jacobian stage begins
  positional_encoding(xc, yc, zc, hh, pe);
  NJF_STAMP_PIN("+v"(pe[0]), "+v"(pe[1]));
  NJF_STAMP(st, 7);  // encoding done
  if (JKIND == 1)
    resnet_tile<PREC, DUMP == 1>(st, bias, gz_j, g, pe, wave, lane, jac, dump);
  else {
    if (DUMP == 1 && dump.pe != nullptr) {  // the transformer head's backward pass recomputes it from pe + footprint
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = pe[kb][4 * q + e];
          *(f32x4*)(dump.pe + 16 * kb + 4 * q) = o;
        }
    }
    // (training forward: dump.act addresses the head's residual-stream dump [4][P][64], render_kernel)
    transformer_tile<PREC>(st, bias, gz_j, g, pe, action_dim, wave, lane, jac, DUMP == 1 ? dump.act : nullptr, dump.stride);
  }
  }
  // flow_s = sum_a J[3a+s] * action[a]  (action_decoder_jacobian.py:128-145); this lane holds
  // logical outputs 16*hh + r.  Partial sums by phase r%3, then the two halves are combined.
  float ph[3] = {0.f, 0.f, 0.f};
  if (action) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d0 = r, d1 = 16 + r;  // logical output index for hh = 0 / 1
      const float a0 = (d0 / 3) < action_dim ? action[d0 / 3] : 0.f;
      const float a1 = (d1 / 3) < action_dim ? action[d1 / 3] : 0.f;
      ph[r % 3] = fmaf(jac[0][r], hh ? a1 : a0, ph[r % 3]);
    }
  }
  // hh=0: spatial index s = r%3 ; hh=1: s = (16+r)%3 = (r+1)%3  ->  phase (s+2)%3
  float mine[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) mine[s] = hh ? ph[(s + 2) % 3] : ph[s];
#pragma unroll
  for (int s = 0; s < 3; ++s) flow[s] = mine[s] + __shfl_xor(mine[s], 32, 64);
}

// =============================================================================================
// final pass: decoder + compositing
// =============================================================================================
struct RenderArgs {
  RayCommon rc;
  int goff_d, goff_j;
  const float* w_all;  // [density 22 chunks | colour 1 | jacobian 22] contiguous
  const float* b_d;
  const float* b_c;
  const float* b_j;
  const float* bins;
  int samples;
  NjfRenderOutputs out;
};

// sample placement of lane j of tile t: interval [start, end], its mid-point and the world-space position there
// (ray_samplers.py:104-147).  Recomputed from the bins after each network instead of being kept in registers.
struct SamplePlace {
  float delta, tm, px, py, pz;
};
// `b0`, `b1`: the sample's two bin edges, loaded once per tile and kept in two registers; the five derived values are
// recomputed where they are needed (opaque copies: otherwise the compiler keeps all five alive across the networks)
__device__ __forceinline__ void place_sample(float b0, float b1, float near, float far, float ox,
                                             float oy, float oz, float dx, float dy, float dz, SamplePlace& sp) {
  asm volatile("" : "+v"(b0), "+v"(b1));
  const float start = b0 * far + (1.0f - b0) * near;
  const float end = b1 * far + (1.0f - b1) * near;
  const float se = start + end;
  sp.delta = end - start;
  sp.tm = se / 2.0f;
  sp.px = ox + (dx * se) / 2.0f;
  sp.py = oy + (dy * se) / 2.0f;
  sp.pz = oz + (dz * se) / 2.0f;
}

// AF: composite the per-sample action features (sum_s w J, 16 more accumulators per lane) -- a compile-time switch
// because the extra live registers cost ~80 spilled VGPRs in the frames that do not ask for them
// PRECJ: MFMA precision of the Jacobian head (default: that of the density / colour networks)
template <int JKIND, int PREC, int DUMP = 0, bool AF = true, int PRECJ = PREC>
__global__ void __launch_bounds__(NJF_THREADS, 2) render_kernel(RenderArgs a) {
  constexpr bool WITH_J = JKIND != 0;
  constexpr int J_CHUNKS = JKIND == 1 ? resnet_chunks<PRECJ>() : (JKIND == 2 ? NJF_TRANSFORMER_CHUNKS : 0);
  constexpr int J_BIAS = JKIND == 1 ? NJF_RESNET_B_FLOATS : NJF_TRANSFORMER_B_FLOATS;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, j = lane & 31, hh = lane >> 5;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int ray = wg * NJF_WAVES + wave;
  const bool ray_ok = ray < a.rc.total_rays;
  const int rayc = min(ray, a.rc.total_rays - 1);
  const int b = rayc / a.rc.rays_per_batch;
  const int S = a.samples;

  load_bias_block(a.b_d, NJF_RESNET_B_FLOATS, 0);
  load_bias_block(a.b_c, NJF_COLOR_B_FLOATS, NJF_RESNET_B_FLOATS);
  if (WITH_J) load_bias_block(a.b_j, J_BIAS, NJF_RESNET_B_FLOATS + NJF_COLOR_B_FLOATS);
  const int tiles = (S + 31) >> 5;
  WeightStreamT<resnet_gap_at<PREC>(), resnet_gap<PREC>()> st;
  stream_begin(st, a.w_all, resnet_chunks<PREC>() + 1 + J_CHUNKS, tiles, wave, lane);
  NJF_STAMP_ARM(st, false, wave);

  CamCtx cam;
  load_ctx(a.rc.cams.ctxt_w2c, a.rc.cams.ctxt_k, b, cam);
  const float near = a.rc.cams.z_near[b], far = a.rc.cams.z_far[b];
  const float ox = a.rc.origins[3 * (size_t)rayc], oy = a.rc.origins[3 * (size_t)rayc + 1],
              oz = a.rc.origins[3 * (size_t)rayc + 2];
  const float dx = a.rc.directions[3 * (size_t)rayc], dy = a.rc.directions[3 * (size_t)rayc + 1],
              dz = a.rc.directions[3 * (size_t)rayc + 2];
  const size_t gbase = (size_t)b * a.rc.gmap.height * a.rc.gmap.width * a.rc.gmap.stride;
  const float* gz_d = map_at<PREC>(a.rc.gmap.data, gbase + a.goff_d);
  const float* gz_j = map_at<PRECJ>(a.rc.gmap.data, gbase + a.goff_j);
  const float* bins = a.bins + (size_t)rayc * (S + 1);
  const int A = a.rc.cams.action_dim;
  const float* action = a.rc.cams.action ? a.rc.cams.action + (size_t)b * A : nullptr;

  float carry = 0.f;
  float acc_rgb[3] = {0.f, 0.f, 0.f}, acc_w = 0.f, acc_wt = 0.f;
  float acc_p[3] = {0.f, 0.f, 0.f}, acc_pw[3] = {0.f, 0.f, 0.f};
  float tmin = 3.0e38f, tmax = -3.0e38f;
  f32x16 acc_j = (f32x16)(0.f);
  const bool want_af = AF && WITH_J && a.out.action_features != nullptr;

  for (int t = 0; t < tiles; ++t) {
    const int s = t * 32 + j;
    const bool valid = s < S;
    const int sc_i = min(s, S - 1);
    const size_t si = (size_t)ray * S + s;
    const bool store = valid && ray_ok;
    const float bin0 = bins[sc_i], bin1 = bins[sc_i + 1];
    PointGeom g;
    {
      SamplePlace sp;
      place_sample(bin0, bin1, near, far, ox, oy, oz, dx, dy, dz, sp);
      point_geometry(cam, sp.px, sp.py, sp.pz, a.rc.gmap.height, a.rc.gmap.width, a.rc.gmap.stride, 0u, g);
    }
    NJF_STAMP(st, 10);  // tile begins
    ActDump dump{nullptr, nullptr, 0};
    ColorDump cdump{nullptr, nullptr, 0};
    if (DUMP != 0 && store) {
      const size_t points = (size_t)a.rc.total_rays * S;
      const NjfActivationDump d{DUMP == 1 ? a.out.jac_act : a.out.den_act, a.out.jac_pe, a.out.foot_idx, a.out.foot_w,
                                DUMP == 1 ? a.out.jac_mask : a.out.den_mask, a.out.dump_f16};
      dump = point_dump(d, si, points, hh, g, b * a.rc.gmap.height * a.rc.gmap.width, a.rc.gmap.stride);
      if constexpr (JKIND == 2 && DUMP == 1) {
        // the transformer head's backward pass (njf_transformer_backward) recomputes each layer from the residual stream in front
        // of it: jac_act is [4][P][64] here -- x before layers 0, 1, 2 and behind layer 2 -- written by transformer_tile
        dump.act = a.out.jac_act ? a.out.jac_act + si * 64 + 32 * hh : nullptr;
        dump.stride = points * 64;
        dump.mask = nullptr;
        dump.half = false;
      }
      if (DUMP == 2) cdump = ColorDump{a.out.col_in + si * 32 + 16 * hh, a.out.col_act + si * 64 + 32 * hh, points * 64};
    }
    // ---- density net -> sample weight; everything that only needs the weight is composited right away
    f32x16 geo[1];
    // plain-fp16 inference: the tile's packed encoding serves both networks, one footprint the gathers of a network (TileShareF16)
#define NJF_F16_SHARE_D 1
#define NJF_F16_SHARE_J 3
    // (the instantiations that also composite the action features, AF, have no registers to spare: 6-35 spilled VGPRs with any of it)
    constexpr int SHARE_D = (PREC == PREC_F16 && DUMP == 0 && !AF) ? NJF_F16_SHARE_D : 0;
    constexpr int SHARE_J = (SHARE_D != 0 && JKIND == 1 && PRECJ == PREC_F16) ? NJF_F16_SHARE_J : 0;
    TileShareF16 share;
    const float sigma = density_stage<PREC, DUMP, SHARE_D>(st, gz_d, g, wave, lane, geo, DUMP == 2 ? dump : ActDump{nullptr, nullptr, 0}, &share);
    float w;
    {
      SamplePlace sp;
      place_sample(bin0, bin1, near, far, ox, oy, oz, dx, dy, dz, sp);
      NJF_STAMP(st, 14);  // density net returned
      w = tile_weights(sp.delta, sigma, valid, j, carry);
      NJF_STAMP_PIN("+v"(w));
      NJF_STAMP(st, 15);  // weights done
      if (valid) {
        acc_w += w;
        acc_wt = fmaf(w, sp.tm, acc_wt);
        tmin = fminf(tmin, sp.tm);
        tmax = fmaxf(tmax, sp.tm);
        acc_p[0] = fmaf(w, sp.px, acc_p[0]);
        acc_p[1] = fmaf(w, sp.py, acc_p[1]);
        acc_p[2] = fmaf(w, sp.pz, acc_p[2]);
      }
    }
    if (store && hh == 0) {
      if (a.out.weights) a.out.weights[si] = w;
      if (a.out.density) a.out.density[si] = sigma;
    }
    // ---- colour head
    NJF_STAMP(st, 11);  // density net + weights done
    {
      float rgb[3];
      color_stage<PREC, DUMP>(st, geo, dx, dy, dz, wave, lane, rgb, cdump);
      if (valid) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc_rgb[c] = fmaf(w, rgb[c], acc_rgb[c]);
      }
      if (store && hh == 0 && a.out.color) {
        a.out.color[3 * si] = rgb[0];
        a.out.color[3 * si + 1] = rgb[1];
        a.out.color[3 * si + 2] = rgb[2];
      }
    }
    // ---- Jacobian head -> scene flow
    NJF_STAMP(st, 12);  // colour head done
    float flow[3] = {0.f, 0.f, 0.f};
    if (WITH_J) {
      f32x16 jac[1];
      jacobian_stage<JKIND, PRECJ, DUMP, SHARE_J>(st, gz_j, g, action, A, wave, lane, jac, flow, DUMP == 1 ? dump : ActDump{nullptr, nullptr, 0}, &share);
      if (valid && want_af) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_j[r] = fmaf(w, jac[0][r], acc_j[r]);
      }
      if (store) {
        if (hh == 0 && a.out.sample_flow) {
          a.out.sample_flow[3 * si] = flow[0];
          a.out.sample_flow[3 * si + 1] = flow[1];
          a.out.sample_flow[3 * si + 2] = flow[2];
        }
        if (a.out.jacobian) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int d = 16 * hh + r;
            if (d < 3 * A) a.out.jacobian[si * (3 * A) + d] = jac[0][r];
          }
        }
      }
    }
    if (valid) {
      SamplePlace sp;
      place_sample(bin0, bin1, near, far, ox, oy, oz, dx, dy, dz, sp);
      acc_pw[0] = fmaf(w, sp.px + flow[0], acc_pw[0]);
      acc_pw[1] = fmaf(w, sp.py + flow[1], acc_pw[1]);
      acc_pw[2] = fmaf(w, sp.pz + flow[2], acc_pw[2]);
    }
  }

  NJF_STAMP_FLUSH(st, 13, lane);  // tiles done
  // reduce over the ray's samples (32 lanes of a half; both halves hold identical per-sample data)
  acc_w = half_sum(acc_w);
  acc_wt = half_sum(acc_wt);
  tmin = half_min(tmin);
  tmax = half_max(tmax);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    acc_rgb[c] = half_sum(acc_rgb[c]);
    acc_p[c] = half_sum(acc_p[c]);
    acc_pw[c] = half_sum(acc_pw[c]);
  }
  if (want_af) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_j[r] = half_sum(acc_j[r]);
    if (ray_ok && j == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int d = 16 * hh + r;
        if (d < 3 * A) a.out.action_features[(size_t)ray * (3 * A) + d] = acc_j[r];
      }
    }
  }
  float flow2d[2] = {0.f, 0.f};
  if (ray_ok && lane == 0) {
    if (a.out.rgb) {
      a.out.rgb[3 * (size_t)ray] = acc_rgb[0];
      a.out.rgb[3 * (size_t)ray + 1] = acc_rgb[1];
      a.out.rgb[3 * (size_t)ray + 2] = acc_rgb[2];
    }
    if (a.out.depth) a.out.depth[ray] = acc_wt / (acc_w + 1e-10f);
    if (a.out.step_minmax) {
      a.out.step_minmax[2 * (size_t)ray] = tmin;
      a.out.step_minmax[2 * (size_t)ray + 1] = tmax;
    }
    if (a.out.pos) {
      a.out.pos[3 * (size_t)ray] = acc_p[0];
      a.out.pos[3 * (size_t)ray + 1] = acc_p[1];
      a.out.pos[3 * (size_t)ray + 2] = acc_p[2];
    }
    if (a.out.pos_warped) {
      a.out.pos_warped[3 * (size_t)ray] = acc_pw[0];
      a.out.pos_warped[3 * (size_t)ray + 1] = acc_pw[1];
      a.out.pos_warped[3 * (size_t)ray + 2] = acc_pw[2];
    }
    if (a.out.flow && a.rc.cams.trgt_w2c && a.rc.cams.trgt_k) {
      // project_world_coords_to_camera (rendering/geometry.py:206-215) of both means
      const float* m = a.rc.cams.trgt_w2c + b * 16;
      const float* k = a.rc.cams.trgt_k + b * 9;
      float uv[2][2];
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const float* p = v ? acc_pw : acc_p;
        const float xc = dot4_h(m + 0, p[0], p[1], p[2]);
        const float yc = dot4_h(m + 4, p[0], p[1], p[2]);
        const float zc = dot4_h(m + 8, p[0], p[1], p[2]);
        const float u0 = dot3(k + 0, xc, yc, zc), u1 = dot3(k + 3, xc, yc, zc), u2 = dot3(k + 6, xc, yc, zc);
        uv[v][0] = u0 / (u2 + 1e-9f);
        uv[v][1] = u1 / (u2 + 1e-9f);
      }
      flow2d[0] = uv[1][0] - uv[0][0];
      flow2d[1] = uv[1][1] - uv[0][1];
      a.out.flow[2 * (size_t)ray] = flow2d[0];
      a.out.flow[2 * (size_t)ray + 1] = flow2d[1];
    }
  }
  if (a.out.frame_partials) {
    // frame-level reductions of this workgroup's four rays (include/njf_hip.h: NjfRenderOutputs.frame_partials), in a fixed
    // order
    float se_rgb = 0.f, se_flow = 0.f;
    if (ray_ok && lane == 0) {
      if (a.out.trgt_rgb && a.out.rgb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float d = acc_rgb[c] - a.out.trgt_rgb[3 * (size_t)ray + c];
          se_rgb = fmaf(d, d, se_rgb);
        }
      }
      if (a.out.trgt_flow && a.out.flow && a.rc.cams.trgt_w2c && a.rc.cams.trgt_k) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const float d = flow2d[c] - a.out.trgt_flow[2 * (size_t)ray + c];
          se_flow = fmaf(d, d, se_flow);
        }
      }
    }
    __syncthreads();  // every wave has consumed its last weight chunk: the weight buffers are free
    if (lane == 0) {
      njf_lds[4 * wave + 0] = ray_ok ? tmin : 3.0e38f;
      njf_lds[4 * wave + 1] = ray_ok ? tmax : -3.0e38f;
      njf_lds[4 * wave + 2] = se_rgb;
      njf_lds[4 * wave + 3] = se_flow;
    }
    __syncthreads();
    if (tid == 0) {
      float mn = njf_lds[0], mx = njf_lds[1], s0 = njf_lds[2], s1 = njf_lds[3];
#pragma unroll
      for (int w = 1; w < NJF_WAVES; ++w) {
        mn = fminf(mn, njf_lds[4 * w]);
        mx = fmaxf(mx, njf_lds[4 * w + 1]);
        s0 += njf_lds[4 * w + 2];
        s1 += njf_lds[4 * w + 3];
      }
      float* dst = a.out.frame_partials + 4 * (size_t)wg;
      dst[0] = mn;
      dst[1] = mx;
      dst[2] = s0;
      dst[3] = s1;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// frame-level reductions of a (ray-sharded) render: fold the per-workgroup partials of the render kernel's epilogue, and
// assemble the frame from the all-gathered per-rank packets (include/njf_hip.h).  Fixed orders: bit-reproducible.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) reduce_frame_partials_kernel(const float* __restrict__ partials, int groups,
                                                                    float* __restrict__ out4) {
  __shared__ float red[4][256];
  float mn = 3.0e38f, mx = -3.0e38f, s0 = 0.f, s1 = 0.f;
  for (int g = threadIdx.x; g < groups; g += 256) {
    const f32x4 v = *(const f32x4*)(partials + 4 * (size_t)g);
    mn = fminf(mn, v[0]);
    mx = fmaxf(mx, v[1]);
    s0 += v[2];
    s1 += v[3];
  }
  red[0][threadIdx.x] = mn;
  red[1][threadIdx.x] = mx;
  red[2][threadIdx.x] = s0;
  red[3][threadIdx.x] = s1;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) {
      red[0][threadIdx.x] = fminf(red[0][threadIdx.x], red[0][threadIdx.x + o]);
      red[1][threadIdx.x] = fmaxf(red[1][threadIdx.x], red[1][threadIdx.x + o]);
      red[2][threadIdx.x] += red[2][threadIdx.x + o];
      red[3][threadIdx.x] += red[3][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) out4[threadIdx.x] = red[threadIdx.x][0];
}

extern "C" int njf_reduce_frame_partials(const float* partials, int groups, float* out4, void* stream) {
  if (!partials || !out4) return NJF_E_NULL;
  if (groups < 1) return NJF_E_SHAPE;
  reduce_frame_partials_kernel<<<1, 256, 0, (hipStream_t)stream>>>(partials, groups, out4);
  return launch_status();
}

__global__ void __launch_bounds__(256) assemble_frame_kernel(const float* __restrict__ packets, int world, int packet_floats,
                                                             int batch, int rays, int cap, float rgb_scale, float flow_scale,
                                                             float* __restrict__ frame, float* __restrict__ scalars6) {
  // global bounds / sums from the trailing record of every packet, ranks in order (every workgroup recomputes them:
  // world <= a few dozen, and it saves a launch)
  float mn = 3.0e38f, mx = -3.0e38f, s0 = 0.f, s1 = 0.f;
  for (int k = 0; k < world; ++k) {
    const float* rec = packets + (size_t)k * packet_floats + (packet_floats - 4);
    mn = fminf(mn, rec[0]);
    mx = fmaxf(mx, rec[1]);
    s0 += rec[2];
    s1 += rec[3];
  }
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    scalars6[0] = mn;
    scalars6[1] = mx;
    scalars6[2] = s0;
    scalars6[3] = s1;
    scalars6[4] = s0 * rgb_scale;    // e.g. 1 / (B*R*3): the photometric mse of the whole frame (model_wrapper.py:119-121)
    scalars6[5] = s1 * flow_scale;   // e.g. 0.01 / (B*R*2): flow_loss (model_wrapper.py:148-160)
  }
  if (i >= (long long)batch * rays) return;
  const int b = (int)(i / rays), r = (int)(i % rays);
  // parallel.shard_bounds: the first `rem` ranks own q + 1 rays, the others q
  const int q = rays / world, rem = rays % world;
  int k, local;
  if (r < rem * (q + 1)) {
    k = r / (q + 1);
    local = r - k * (q + 1);
  } else {
    k = rem + (r - rem * (q + 1)) / max(q, 1);
    local = r - rem * (q + 1) - (k - rem) * q;
  }
  const int n_k = q + (k < rem ? 1 : 0);
  const float* pk = packets + (size_t)k * packet_floats;
  const float* rgb = pk + ((size_t)b * n_k + local) * 3;
  const float* dep = pk + (size_t)3 * batch * cap + (size_t)b * n_k + local;
  const float* flw = pk + (size_t)4 * batch * cap + ((size_t)b * n_k + local) * 2;
  float* dst = frame + (size_t)i * 6;
  dst[0] = rgb[0];
  dst[1] = rgb[1];
  dst[2] = rgb[2];
  dst[3] = fminf(fmaxf(dep[0], mn), mx);   // torch.clip(depth, steps.min(), steps.max()) with the GLOBAL bounds
  dst[4] = flw[0];
  dst[5] = flw[1];
}

extern "C" int njf_assemble_frame(const float* packets, int world, int packet_floats, int batch, int rays_per_batch,
                                  float rgb_scale, float flow_scale, float* frame, float* scalars6, void* stream) {
  if (!packets || !frame || !scalars6) return NJF_E_NULL;
  if (world < 1 || batch < 1 || rays_per_batch < 1) return NJF_E_SHAPE;
  const int cap = (rays_per_batch + world - 1) / world;
  if (packet_floats < 6 * batch * cap + 4) return NJF_E_SHAPE;
  const long long total = (long long)batch * rays_per_batch;
  assemble_frame_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(packets, world, packet_floats, batch,
                                                                                          rays_per_batch, cap, rgb_scale, flow_scale,
                                                                                          frame, scalars6);
  return launch_status();
}

// a length that lives on the device: min(*count, capacity), the capacity without a count (what a capture-safe caller launches for)
__device__ __forceinline__ int counted_length(const int* count, int capacity) {
  return count ? min(max(*count, 0), capacity) : capacity;
}

// =============================================================================================
// voxel-grid field extraction: grid-driven point evaluator, ordered selection, coordinates
// =============================================================================================
// Node (ix, iy, iz) of a grid (NjfFieldGrid) has linear index n = (ix*ny + iy)*nz + iz and the coordinate
// fmaf(i_c, step[c], origin[c]); node n of batch element b has the GLOBAL index b*N + n (N = nx*ny*nz, B*N < 2^31).
// A "list" is `indices` (global indices, NULL = the identity) with its entry count min(*count, capacity) read from device
// memory (count NULL = capacity): a capture-safe caller launches for the capacity, surplus workgroups leave at once.
struct FieldList {
  NjfFieldGrid grid;
  int nodes;           // N
  int total;           // B*N
  const int* indices;  // or null
  const int* count;    // or null
  int capacity;
};

__device__ __forceinline__ int field_entries(const FieldList& l) {
  return counted_length(l.count, l.capacity);
}

// global index of list entry i, clamped into the grid (an index list is caller data: nothing may address outside the
// cameras / the hoisted map because of it)
__device__ __forceinline__ int field_global_index(const FieldList& l, int i) {
  const int gi = l.indices ? l.indices[i] : i;
  return min(max(gi, 0), l.total - 1);
}

// the coordinate of the node of linear index n
__device__ __forceinline__ void grid_node(const NjfFieldGrid& grid, int n, float& px, float& py, float& pz) {
  const int yz = grid.dims[1] * grid.dims[2];
  const int ix = n / yz, r = n - ix * yz;
  const int iy = r / grid.dims[2], iz = r - iy * grid.dims[2];
  px = fmaf((float)ix, grid.step[0], grid.origin[0]);
  py = fmaf((float)iy, grid.step[1], grid.origin[1]);
  pz = fmaf((float)iz, grid.step[2], grid.origin[2]);
}

__device__ __forceinline__ void field_node(const FieldList& l, int gi, int& b, float& px, float& py, float& pz) {
  b = gi / l.nodes;
  grid_node(l.grid, gi - b * l.nodes, px, py, pz);
}

// ---- the decoder at points: one evaluator, three sources of points ------------------------------------------------------
// What every source shares; the last three outputs exist for the point list alone (SRC::EXTRAS).
struct DecoderArgs {
  NjfCameras cams;
  NjfFeatureMap gmap;
  int goff_d, goff_j;
  const float* w_all;
  const float* b_d;
  const float* b_c;
  const float* b_j;
  float* density;   // [entries] or null
  float* color;     // [entries, 3] or null
  float* jacobian;  // [entries, 3A] or null
  float* flow;      // [entries, 3] or null
  float* geo;       // [entries, 15] or null
  float* features;  // [5, entries, 128] or null (FEAT instantiation only)
};

// A source says how many entries there are, which batch element and position entry i has, and the view direction of its
// colour head.  COUNTED: the entry count lives on the device (surplus workgroups leave at once); EXTRAS: the per-lane action
// (hence `flow`), `geo` and the feature dump; MODES: bit m = the source has evaluator MODE m.
struct PointList {  // njf_points_forward
  static constexpr bool COUNTED = false, EXTRAS = true;
  static constexpr int MODES = 0b11101;
  const float* xyz;
  const float* dirs;  // or null
  int points_per_batch;
  int total;
  __device__ __forceinline__ int entries() const { return total; }
  __device__ __forceinline__ void point(int i, int& b, float& px, float& py, float& pz) const {
    b = i / points_per_batch;  // per lane: a tile may straddle batch elements
    px = xyz[3 * (size_t)i], py = xyz[3 * (size_t)i + 1], pz = xyz[3 * (size_t)i + 2];
  }
  __device__ __forceinline__ void direction(int i, float& dx, float& dy, float& dz) const {
    dx = 0.f, dy = 0.f, dz = 1.f;
    if (dirs) dx = dirs[3 * (size_t)i], dy = dirs[3 * (size_t)i + 1], dz = dirs[3 * (size_t)i + 2];
  }
};
struct ConstantDirection {
  float dirx, diry, dirz;
  __device__ __forceinline__ void direction(int, float& dx, float& dy, float& dz) const { dx = dirx, dy = diry, dz = dirz; }
};
struct GridNodes : ConstantDirection {  // njf_field_forward: row i of every output is list entry i
  static constexpr bool COUNTED = true, EXTRAS = false;
  static constexpr int MODES = 0b11111;
  FieldList list;
  __device__ __forceinline__ int entries() const { return field_entries(list); }
  __device__ __forceinline__ void point(int i, int& b, float& px, float& py, float& pz) const {
    field_node(list, field_global_index(list, i), b, px, py, pz);
  }
};
struct StoredNodes : ConstantDirection {  // njf_field_forward_at (the mesh vertices): a ragged batch in one launch
  static constexpr bool COUNTED = true, EXTRAS = false;
  static constexpr int MODES = 0b11100;
  const float* xyz;  // [capacity, 3]
  const int* node;   // [capacity] global node index: the batch element of row i is node[i] / nodes
  const int* count;  // or null
  int capacity;
  int nodes, total;  // N, B*N
  __device__ __forceinline__ int entries() const { return counted_length(count, capacity); }
  __device__ __forceinline__ void point(int i, int& b, float& px, float& py, float& pz) const {
    b = min(max(node[i], 0), total - 1) / nodes;  // (caller data: clamped into the batch)
    px = xyz[3 * (size_t)i], py = xyz[3 * (size_t)i + 1], pz = xyz[3 * (size_t)i + 2];
  }
};

// MODE 0: proposal net; 1: decoder density only (the density net alone is streamed); 2: density + colour; 3: density +
// colour + ResnetFC Jacobian head; 4: density + colour + transformer Jacobian head.  FEAT (MODE 3): the head also stores
// its residual stream after every block (ResnetFC.forward(compute_features=True), resnet_fc.py:141-151) through the
// training instantiation of resnet_tile.  One body for every source: a row's outputs are the same function of its
// position, batch element and view direction whichever entry point evaluates it.
template <class SRC, int MODE, int PREC, int PRECJ = PREC, bool FEAT = false>
__global__ void __launch_bounds__(NJF_THREADS, 2) points_kernel(DecoderArgs a, SRC src) {
  static_assert((SRC::MODES >> MODE) & 1, "a mode this source does not have");
  const int entries = src.entries();
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, j = lane & 31, hh = lane >> 5;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  if (SRC::COUNTED && wg * (NJF_WAVES * 32) >= entries) return;  // the whole workgroup (it shares the weight stream), before any barrier
  const int tile = wg * NJF_WAVES + wave;
  const int p = tile * 32 + j;
  const bool ok = p < entries;
  const int pc = min(p, entries - 1);

  load_bias_block(a.b_d, NJF_RESNET_B_FLOATS, 0);
  if (MODE >= 2) load_bias_block(a.b_c, NJF_COLOR_B_FLOATS, NJF_RESNET_B_FLOATS);
  if (MODE == 3) load_bias_block(a.b_j, NJF_RESNET_B_FLOATS, NJF_RESNET_B_FLOATS + NJF_COLOR_B_FLOATS);
  if (MODE == 4) load_bias_block(a.b_j, NJF_TRANSFORMER_B_FLOATS, NJF_RESNET_B_FLOATS + NJF_COLOR_B_FLOATS);
  WeightStreamT<resnet_gap_at<PREC>(), resnet_gap<PREC>()> st;
  stream_begin(st, a.w_all,
               MODE <= 1 ? resnet_chunks<PREC>()
                         : resnet_chunks<PREC>() + 1 + (MODE == 3 ? resnet_chunks<PRECJ>() : (MODE == 4 ? NJF_TRANSFORMER_CHUNKS : 0)),
               1, wave, lane);
  int b;
  float px, py, pz;
  src.point(pc, b, px, py, pz);
  CamCtx cam;
  load_ctx(a.cams.ctxt_w2c, a.cams.ctxt_k, b, cam);
  PointGeom g;
  // the batch element's offset travels with the point (PointGeom::gofs): the gathers take the map itself as base
  const unsigned gbase = (unsigned)b * (unsigned)(a.gmap.height * a.gmap.width) * (unsigned)a.gmap.stride;
  point_geometry(cam, px, py, pz, a.gmap.height, a.gmap.width, a.gmap.stride, gbase, g);
  const float* bias = njf_lds + LDS_BIAS;
  if (MODE == 0) {
    f32x16 pe[2], out[1];
    positional_encoding(g.xc, g.yc, g.zc, hh, pe);
    resnet_tile<PREC>(st, bias, map_at<PREC>(a.gmap.data, a.goff_d), g, pe, wave, lane, out);
    if (ok && hh == 0 && (!SRC::EXTRAS || a.density)) a.density[p] = expf(out[0][0] - 1.0f);  // (mandatory but for the point list)
  } else {
    const int A = a.cams.action_dim;
    constexpr int JK = MODE >= 3 ? MODE - 2 : 0;
    const ActDump nodump{nullptr, nullptr, 0};
    // stage by stage, each result stored before the next network starts (nothing but the point itself stays live)
    f32x16 geo[1];
    const float sigma = density_stage<PREC, 0>(st, map_at<PREC>(a.gmap.data, a.goff_d), g, wave, lane, geo, nodump);
    if (ok && hh == 0) {
      if (a.density) a.density[p] = sigma;
      if (SRC::EXTRAS && a.geo) {
#pragma unroll
        for (int r = 0; r < 15; ++r) a.geo[15 * (size_t)p + r] = geo[0][r];
      }
    }
    if (MODE >= 2) {
      float dx, dy, dz, rgb[3];
      src.direction(pc, dx, dy, dz);
      color_stage<PREC, 0>(st, geo, dx, dy, dz, wave, lane, rgb, ColorDump{nullptr, nullptr, 0});
      if (ok && hh == 0 && a.color) {
        a.color[3 * (size_t)p] = rgb[0];
        a.color[3 * (size_t)p + 1] = rgb[1];
        a.color[3 * (size_t)p + 2] = rgb[2];
      }
    }
    if (JK != 0) {
      f32x16 jac[1];
      float flow[3];
      // per lane (tiles may straddle batch elements); a literal null without EXTRAS: no flow arithmetic is compiled
      const float* action = SRC::EXTRAS && a.cams.action ? a.cams.action + (size_t)b * A : nullptr;
      if constexpr (FEAT) {
        static_assert(MODE == 3 && SRC::EXTRAS, "feature dump: ResnetFC head of the point list");
        ActDump fdump{nullptr, nullptr, (size_t)entries * 128};
        if (ok) fdump.feat = a.features + (size_t)p * 128 + 64 * hh;
        jacobian_stage<JK, PRECJ, 1>(st, map_at<PRECJ>(a.gmap.data, a.goff_j), g, action, A, wave, lane, jac, flow, fdump);
      } else
      jacobian_stage<JK, PRECJ, 0>(st, map_at<PRECJ>(a.gmap.data, a.goff_j), g, action, A, wave, lane, jac, flow, nodump);
      if (ok) {
        if (SRC::EXTRAS && hh == 0 && a.flow) {
          a.flow[3 * (size_t)p] = flow[0];
          a.flow[3 * (size_t)p + 1] = flow[1];
          a.flow[3 * (size_t)p + 2] = flow[2];
        }
        if (a.jacobian) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int d = 16 * hh + r;
            if (d < 3 * A) a.jacobian[(size_t)p * (3 * A) + d] = jac[0][r];
          }
        }
      }
    }
  }
}

// xyz [entries, 3]: the coordinates of a list's nodes (the very floats points_kernel<GridNodes> evaluates)
__global__ void __launch_bounds__(256) field_xyz_kernel(FieldList l, float* __restrict__ xyz) {
  const int entries = field_entries(l);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= entries) return;
  int b;
  float px, py, pz;
  field_node(l, field_global_index(l, i), b, px, py, pz);
  xyz[3 * (size_t)i] = px;
  xyz[3 * (size_t)i + 1] = py;
  xyz[3 * (size_t)i + 2] = pz;
}

// ---- workgroup sums, ranks and offsets -------------------------------------------------------------
// What the field entries share when they count, rank or compact the entries of a workgroup.  A thread holds ITEMS entries:
// item `it` of thread tid is entry it * blockDim.x + tid, so the order inside a workgroup is item-major, then wave, then lane
// -- ascending index.  Integer arithmetic, no atomics, every order fixed by (ITEMS, WAVES) alone: what comes out of these
// is a function of the inputs, never of scheduling.  Every thread of the workgroup calls (barriers inside); `lds` is free
// again after a barrier of the caller.
//
// the butterfly 32, 16, ..., 1: every lane ends with the wave's sum.  The offset order is part of the contract -- the double
// sums of the twists, the commands and the compositing backward are compared bit for bit (a + b == b + a bit for bit, so
// every lane holds the same bits).
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the workgroup's sum of the per-wave totals `n` (wave-uniform: a ballot + popcount count stays on the scalar unit)
template <int WAVES>
__device__ __forceinline__ int block_sum_waves(int n, int (&lds)[WAVES]) {
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = n;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) s += lds[w];
  return s;
}

// the workgroup's sum of `v`
template <int WAVES>
__device__ __forceinline__ int block_sum(int v, int (&lds)[WAVES]) {
  return block_sum_waves(wave_sum(v), lds);
}

// bit `it` of `flags`: item `it` is kept.  f(it, rank) for every kept item, `it` ascending, with rank = base + the kept
// entries of the workgroup in front of the item (its place in the ordered output); returns the workgroup's number of kept
// entries.  (A callback, not rank[ITEMS]: with the 16 items of a twist chunk the array cost 50 VGPRs and three waves per SIMD.)
template <int ITEMS, int WAVES, class F>
__device__ __forceinline__ int block_flag_ranks(unsigned flags, int base, int (&lds)[ITEMS][WAVES], F&& f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const unsigned long long m = __ballot((flags >> it) & 1u);
    if (lane == 0) lds[it][wave] = __popcll(m);
  }
  __syncthreads();
  int run = base;
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    int off = run;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const int c = lds[it][w];
      if (w < wave) off += c;
      run += c;
    }
    const unsigned long long m = __ballot((flags >> it) & 1u);  // (again: cheaper than ITEMS masks across the barrier)
    if ((flags >> it) & 1u) f(it, off + __popcll(m & ((1ull << lane) - 1ull)));
  }
  return run - base;
}

// the same for integer counts: rank[it] = base + the sum of c over the workgroup's entries in front of item `it`
template <int ITEMS, int WAVES>
__device__ __forceinline__ void block_count_ranks(const int (&c)[ITEMS], int base, int (&rank)[ITEMS], int (&lds)[ITEMS][WAVES]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int before[ITEMS];
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    int v = c[it];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(v, d, 64);
      if (lane >= d) v += o;
    }
    before[it] = v - c[it];
    if (lane == 63) lds[it][wave] = v;
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    int r = base;
    for (int w = 0; w < wave; ++w) r += lds[it][w];
    rank[it] = r + before[it];
    for (int w = 0; w < WAVES; ++w) base += lds[it][w];
  }
}

// the workgroup of the kernels over blocks of 1,024 consecutive entries (selection, mesh, fusion, band)
#define NJF_BLOCK_THREADS 256
#define NJF_BLOCK_WAVES (NJF_BLOCK_THREADS / 64)
#define NJF_BLOCK_ITEMS (NJF_FIELD_SELECT_BLOCK / NJF_BLOCK_THREADS)
static_assert(NJF_BLOCK_ITEMS * NJF_BLOCK_THREADS == NJF_FIELD_SELECT_BLOCK && NJF_BLOCK_ITEMS <= 8 &&
                  NJF_FIELD_MESH_BLOCK == NJF_FIELD_SELECT_BLOCK && NJF_FIELD_BAND_BLOCK == NJF_FIELD_SELECT_BLOCK,
              "one block of entries");

// one workgroup: the per-workgroup sums at sums[b * STRIDE], b < blocks -> their exclusive prefix sums in place, the
// grand total to *total.  A contiguous run of sums per thread, thread 0 scans the 256 run sums.  (STRIDE at compile time:
// with a run-time stride the strided loads lost their unrolling, 1 to 2 % of the cell list's build.)
template <long long STRIDE>
__global__ void __launch_bounds__(NJF_BLOCK_THREADS) block_offsets_kernel(int* sums, int blocks, int* total) {
  constexpr long long stride = STRIDE;
  __shared__ int part[NJF_BLOCK_THREADS];
  const int t = threadIdx.x;
  const int per = (blocks + NJF_BLOCK_THREADS - 1) / NJF_BLOCK_THREADS;
  const int lo = min(t * per, blocks), hi = min(lo + per, blocks);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += sums[i * stride];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int i = 0; i < NJF_BLOCK_THREADS; ++i) {
      const int c = part[i];
      part[i] = run;
      run += c;
    }
    *total = run;
  }
  __syncthreads();
  int run = part[t];
  for (int i = lo; i < hi; ++i) {
    const int c = sums[i * stride];
    sums[i * stride] = run;
    run += c;
  }
}

// ---- ordered selection --------------------------------------------------------------------
// keep(entry i) = (values == null || values[i] >= threshold) && (no cameras || the node projects inside the context image
// with positive camera depth).  Three launches: per-workgroup counts, block_offsets_kernel, a scatter that re-evaluates the
// predicate and writes the survivors' global indices in input order (block_flag_ranks).
struct SelectArgs {
  FieldList list;
  const float* values;  // [entries] or null
  float threshold;
  const float* w2c;     // [B,4,4] or null (no frustum test)
  const float* k;       // [B,3,3]
  int* out_indices;
  int* out_count;
  int out_capacity;
  int* block_counts;    // [blocks]: counts, then (after the scan) exclusive offsets
  int blocks;
};

// the projection of point_geometry + point_footprint (u, v: normalised image coordinates of the feature gather)
__device__ __forceinline__ bool point_in_view(const CamCtx& cam, float px, float py, float pz) {
  const float xc = dot4_h(cam.m + 0, px, py, pz), yc = dot4_h(cam.m + 4, px, py, pz), zc = dot4_h(cam.m + 8, px, py, pz);
  const float u0 = dot3(cam.k + 0, xc, yc, zc), u1 = dot3(cam.k + 3, xc, yc, zc), u2 = dot3(cam.k + 6, xc, yc, zc);
  const float inv = __builtin_amdgcn_rcpf(u2 + 1e-9f);
  const float u = u0 * inv, v = u1 * inv;
  return zc > 0.0f && u >= 0.0f && u <= 1.0f && v >= 0.0f && v <= 1.0f;  // (NaN compares false)
}

__device__ __forceinline__ bool field_in_view(const SelectArgs& a, int gi) {
  int b;
  float px, py, pz;
  field_node(a.list, gi, b, px, py, pz);
  CamCtx cam;
  load_ctx(a.w2c, a.k, b, cam);
  return point_in_view(cam, px, py, pz);
}

// bit `it` of the result: keep entry block*NJF_FIELD_SELECT_BLOCK + it*NJF_BLOCK_THREADS + tid
__device__ __forceinline__ unsigned select_flags(const SelectArgs& a, int entries) {
  unsigned flags = 0;
#pragma unroll
  for (int it = 0; it < NJF_BLOCK_ITEMS; ++it) {
    const long long i = (long long)blockIdx.x * NJF_FIELD_SELECT_BLOCK + it * NJF_BLOCK_THREADS + threadIdx.x;
    bool keep = i < entries;
    if (keep && a.values) keep = a.values[i] >= a.threshold;
    if (keep && a.w2c) keep = field_in_view(a, field_global_index(a.list, (int)i));
    flags |= keep ? 1u << it : 0u;
  }
  return flags;
}

__global__ void __launch_bounds__(NJF_BLOCK_THREADS) select_count_kernel(SelectArgs a) {
  __shared__ int wave_count[NJF_BLOCK_WAVES];
  const unsigned flags = select_flags(a, field_entries(a.list));
  int n = 0;
#pragma unroll
  for (int it = 0; it < NJF_BLOCK_ITEMS; ++it) n += __popcll(__ballot((flags >> it) & 1u));  // wave-uniform
  const int s = block_sum_waves(n, wave_count);
  if (threadIdx.x == 0) a.block_counts[blockIdx.x] = s;
}

__global__ void __launch_bounds__(NJF_BLOCK_THREADS) select_scatter_kernel(SelectArgs a) {
  __shared__ int wave_count[NJF_BLOCK_ITEMS][NJF_BLOCK_WAVES];
  const unsigned flags = select_flags(a, field_entries(a.list));
  block_flag_ranks(flags, a.block_counts[blockIdx.x], wave_count, [&](int it, int rank) {
    const int i = blockIdx.x * NJF_FIELD_SELECT_BLOCK + it * NJF_BLOCK_THREADS + threadIdx.x;
    if (rank < a.out_capacity) a.out_indices[rank] = field_global_index(a.list, i);
  });
}

// ---- isosurface mesh of a scalar on the grid: marching tetrahedra on the Kuhn cut ------------------------------------------
// inside(g) = values[g] >= threshold (NaN: outside).  Every cell is cut into the six tetrahedra around its main diagonal,
// one per axis order (a, b, c) in the order xyz, xzy, yxz, yzx, zxy, zyx with the corners c0 = (0,0,0), c1 = c0 + e_a,
// c2 = c1 + e_b, c3 = (1,1,1): the cut is translation invariant, so neighbouring cells agree on every face diagonal.  Every
// tetrahedron edge is (lower node) + one of the seven directions k = 0..6 below; the lower node OWNS the edge.  One vertex
// per edge whose ends are both valid and differ in `inside`, in ascending (owner, k); triangles per cell in ascending global
// cell index, tetrahedra in the order above.  Six launches (mask + count, scan, vertex emit; count, scan, triangle emit),
// integer arithmetic apart from the interpolation; sums, ranks and offsets by the workgroup primitives above.
#define NJF_MESH_VALID 0x80u  // bit 7 of a node's mask byte: the node is valid; bits 0..6: edge k carries a vertex
struct MeshArgs {
  SelectArgs sel;              // list: the identity over B*N; values, threshold; w2c / k: frustum part of `valid` (or null)
  const unsigned char* valid;  // [B*N] or null
  unsigned char* mask;         // [B*N]
  int* offset;                 // [B*N] exclusive vertex offset of a node
  int* vertex_node;            // [max_vertices]
  unsigned char* vertex_edge;  // [max_vertices]
  float* vertex_t;             // [max_vertices]
  float* vertices;             // [max_vertices, 3]
  int max_vertices;
  int* triangles;              // [max_triangles, 3]
  int* triangle_cell;          // [max_triangles]
  int max_triangles;
  int cells, total_cells;      // Nc = (nx-1)(ny-1)(nz-1), B*Nc
  int* block_counts;           // per workgroup: counts, then (after the scan) exclusive offsets
};

// corner / direction codes: bit 0 = +x, bit 1 = +y, bit 2 = +z.  Direction k of the edge list -> code, and back
__device__ __forceinline__ int mesh_dir_code(int k) { return (int)((0x7653421u >> (4 * k)) & 7u); }   // 1,2,4,3,5,6,7
__device__ __forceinline__ int mesh_dir_index(int code) { return (int)((0x65423100u >> (4 * code)) & 7u); }  // -,0,1,3,2,4,5,6
__device__ __forceinline__ int mesh_code_offset(const NjfFieldGrid& g, int code) {
  return (code & 1) * g.dims[1] * g.dims[2] + ((code >> 1) & 1) * g.dims[2] + (code >> 2);
}

__device__ __forceinline__ bool mesh_node_valid(const MeshArgs& a, int gi) {
  if (a.valid && a.valid[gi] == 0) return false;
  return a.sel.w2c ? field_in_view(a.sel, gi) : true;
}

// launch 1: the mask byte of every node and the number of vertices per workgroup
__global__ void __launch_bounds__(NJF_BLOCK_THREADS) mesh_mask_kernel(MeshArgs a) {
  __shared__ int wave_part[NJF_BLOCK_WAVES];
  const NjfFieldGrid& g = a.sel.list.grid;
  int n_vertices = 0;
#pragma unroll
  for (int it = 0; it < NJF_BLOCK_ITEMS; ++it) {
    const long long i = (long long)blockIdx.x * NJF_FIELD_MESH_BLOCK + it * NJF_BLOCK_THREADS + threadIdx.x;
    if (i >= a.sel.list.total) continue;
    const int gi = (int)i;
    const int n = gi % a.sel.list.nodes;
    const int yz = g.dims[1] * g.dims[2];
    const int ix = n / yz, r = n - ix * yz;
    const int iy = r / g.dims[2], iz = r - iy * g.dims[2];
    const bool ok0 = mesh_node_valid(a, gi);
    const bool in0 = a.sel.values[gi] >= a.sel.threshold;
    unsigned m = ok0 ? NJF_MESH_VALID : 0u;
    if (ok0) {
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const int code = mesh_dir_code(k);
        if (ix + (code & 1) >= g.dims[0] || iy + ((code >> 1) & 1) >= g.dims[1] || iz + (code >> 2) >= g.dims[2]) continue;
        const int g1 = gi + mesh_code_offset(g, code);
        if ((a.sel.values[g1] >= a.sel.threshold) != in0 && mesh_node_valid(a, g1)) m |= 1u << k;
      }
    }
    a.mask[gi] = (unsigned char)m;
    n_vertices += __popc(m & 0x7fu);
  }
  const int s = block_sum(n_vertices, wave_part);
  if (threadIdx.x == 0) a.block_counts[blockIdx.x] = s;
}

// launch 3: per-node exclusive offsets (all nodes) and the vertex rows of ranks below the capacity
__global__ void __launch_bounds__(NJF_BLOCK_THREADS) mesh_vertex_kernel(MeshArgs a) {
  __shared__ int wave_part[NJF_BLOCK_ITEMS][NJF_BLOCK_WAVES];
  const NjfFieldGrid& g = a.sel.list.grid;
  int c[NJF_BLOCK_ITEMS], rank[NJF_BLOCK_ITEMS];
  unsigned m[NJF_BLOCK_ITEMS];
#pragma unroll
  for (int it = 0; it < NJF_BLOCK_ITEMS; ++it) {
    const long long i = (long long)blockIdx.x * NJF_FIELD_MESH_BLOCK + it * NJF_BLOCK_THREADS + threadIdx.x;
    m[it] = i < a.sel.list.total ? (a.mask[i] & 0x7fu) : 0u;
    c[it] = __popc(m[it]);
  }
  block_count_ranks(c, a.block_counts[blockIdx.x], rank, wave_part);
#pragma unroll
  for (int it = 0; it < NJF_BLOCK_ITEMS; ++it) {
    const long long i = (long long)blockIdx.x * NJF_FIELD_MESH_BLOCK + it * NJF_BLOCK_THREADS + threadIdx.x;
    if (i >= a.sel.list.total) continue;
    const int gi = (int)i;
    a.offset[gi] = rank[it];
    if (m[it] == 0u || rank[it] >= a.max_vertices) continue;
    int b;
    float x0[3];
    field_node(a.sel.list, gi, b, x0[0], x0[1], x0[2]);
    const float v0 = a.sel.values[gi];
    int r = rank[it];
    for (int k = 0; k < 7; ++k) {
      if (!((m[it] >> k) & 1u)) continue;
      if (r < a.max_vertices) {
        const int code = mesh_dir_code(k);
        const int g1 = gi + mesh_code_offset(g, code);
        float x1[3];
        field_node(a.sel.list, g1, b, x1[0], x1[1], x1[2]);
        const float v1 = a.sel.values[g1];
        float t = __fdiv_rn(a.sel.threshold - v0, v1 - v0);  // IEEE division
        if (!__builtin_isfinite(t)) t = 0.5f;                // (an infinite or NaN end)
        t = t > 0.0f ? t : 0.0f;
        t = t < 1.0f ? t : 1.0f;
        a.vertex_node[r] = gi;
        a.vertex_edge[r] = (unsigned char)k;
        a.vertex_t[r] = t;
#pragma unroll
        for (int d = 0; d < 3; ++d) a.vertices[3 * (size_t)r + d] = fmaf(t, x1[d] - x0[d], x0[d]);
      }
      ++r;
    }
  }
}

// the triangles of one cell: `emit(v0, v1, v2)` per triangle in order, vertex ranks; returns their number (0..12).
// COUNT: only the number.  Winding: the normal points from inside to outside, decided by the case and the parity of the
// axis order alone -- with the corner list p = (the inside corners ascending, then the outside ones; for three inside
// corners the outside one first) the sign of det[p1-p0, p2-p0, p3-p0] is (parity of the axis order) * (parity of p).
template <bool COUNT, class F>
__device__ __forceinline__ int mesh_cell_triangles(const MeshArgs& a, int gc, F&& emit) {
  const NjfFieldGrid& g = a.sel.list.grid;
  const int b = gc / a.cells, local = gc - b * a.cells;
  const int cz = g.dims[2] - 1, cy = g.dims[1] - 1;
  const int iz = local % cz, q = local / cz;
  const int iy = q % cy, ix = q / cy;
  const int g0 = b * a.sel.list.nodes + (ix * g.dims[1] + iy) * g.dims[2] + iz;
  unsigned in8 = 0, ok8 = 0;
#pragma unroll
  for (int code = 0; code < 8; ++code) {
    const int gi = g0 + mesh_code_offset(g, code);
    ok8 |= (a.mask[gi] & NJF_MESH_VALID) ? 1u << code : 0u;
    in8 |= a.sel.values[gi] >= a.sel.threshold ? 1u << code : 0u;
  }
  int n_tri = 0;
#pragma unroll
  for (int tet = 0; tet < 6; ++tet) {
    const int ax = tet >> 1, bx = (0x102021 >> (4 * tet)) & 3;  // axis order (a, b, .): xyz xzy yxz yzx zxy zyx
    const int cm[4] = {0, 1 << ax, (1 << ax) | (1 << bx), 7};
    // parity of the axis order: xyz +, xzy -, yxz -, yzx +, zxy +, zyx -
    const bool even_axes = tet == 0 || tet == 3 || tet == 4;
    unsigned inm = 0;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      ok = ok && ((ok8 >> cm[c]) & 1u);
      inm |= ((in8 >> cm[c]) & 1u) << c;
    }
    const int n_in = __popc(inm);
    if (!ok || n_in == 0 || n_in == 4) continue;
    if constexpr (COUNT) {
      n_tri += n_in == 2 ? 2 : 1;
      continue;
    }
    const unsigned lead = n_in == 3 ? (~inm & 15u) : inm;     // the corners listed first
    int p[4], np = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if ((lead >> c) & 1u) p[np++] = c;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (!((lead >> c) & 1u)) p[np++] = c;
    int inversions = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = i + 1; j < 4; ++j) inversions += p[i] > p[j];
    const bool positive = (even_axes == ((inversions & 1) == 0)) != (n_in == 3);
    auto rank_of = [&](int ci, int cj) {  // vertex rank of the edge between local corners ci and cj
      const int lo = min(ci, cj), hi = max(ci, cj);
      const int gi = g0 + mesh_code_offset(g, cm[lo]);
      const int k = mesh_dir_index(cm[hi] ^ cm[lo]);
      return a.offset[gi] + __popc(a.mask[gi] & ((1u << k) - 1u));
    };
    if (n_in != 2) {
      const int v0 = rank_of(p[0], p[1]), v1 = rank_of(p[0], p[2]), v2 = rank_of(p[0], p[3]);
      if (positive) emit(v0, v1, v2); else emit(v0, v2, v1);
      n_tri += 1;
    } else {
      const int ik = rank_of(p[0], p[2]), il = rank_of(p[0], p[3]), jl = rank_of(p[1], p[3]), jk = rank_of(p[1], p[2]);
      if (positive) {
        emit(ik, il, jl);
        emit(ik, jl, jk);
      } else {
        emit(ik, jl, il);
        emit(ik, jk, jl);
      }
      n_tri += 2;
    }
  }
  return n_tri;
}

// launch 4: the number of triangles per workgroup of cells
__global__ void __launch_bounds__(NJF_BLOCK_THREADS) mesh_triangle_count_kernel(MeshArgs a) {
  __shared__ int wave_part[NJF_BLOCK_WAVES];
  int n = 0;
#pragma unroll
  for (int it = 0; it < NJF_BLOCK_ITEMS; ++it) {
    const long long i = (long long)blockIdx.x * NJF_FIELD_MESH_BLOCK + it * NJF_BLOCK_THREADS + threadIdx.x;
    if (i < a.total_cells) n += mesh_cell_triangles<true>(a, (int)i, [](int, int, int) {});
  }
  const int s = block_sum(n, wave_part);
  if (threadIdx.x == 0) a.block_counts[blockIdx.x] = s;
}

// launch 6: the triangle rows of ranks below the capacity
__global__ void __launch_bounds__(NJF_BLOCK_THREADS) mesh_triangle_kernel(MeshArgs a) {
  __shared__ int wave_part[NJF_BLOCK_ITEMS][NJF_BLOCK_WAVES];
  int c[NJF_BLOCK_ITEMS], rank[NJF_BLOCK_ITEMS];
#pragma unroll
  for (int it = 0; it < NJF_BLOCK_ITEMS; ++it) {
    const long long i = (long long)blockIdx.x * NJF_FIELD_MESH_BLOCK + it * NJF_BLOCK_THREADS + threadIdx.x;
    c[it] = i < a.total_cells ? mesh_cell_triangles<true>(a, (int)i, [](int, int, int) {}) : 0;
  }
  block_count_ranks(c, a.block_counts[blockIdx.x], rank, wave_part);
#pragma unroll
  for (int it = 0; it < NJF_BLOCK_ITEMS; ++it) {
    if (c[it] == 0 || rank[it] >= a.max_triangles) continue;
    const int gc = blockIdx.x * NJF_FIELD_MESH_BLOCK + it * NJF_BLOCK_THREADS + threadIdx.x;
    int r = rank[it];
    mesh_cell_triangles<false>(a, gc, [&](int v0, int v1, int v2) {
      if (r < a.max_triangles) {
        a.triangles[3 * (size_t)r] = v0;
        a.triangles[3 * (size_t)r + 1] = v1;
        a.triangles[3 * (size_t)r + 2] = v2;
        a.triangle_cell[r] = gc;
      }
      ++r;
    });
  }
}

// ---- fusion of the fields of several context views ------------------------------------------------
// The B context images are G = B / V scenes of V consecutive views (batch element b = g*V + v) on one grid.  s_v = the frustum
// predicate of the selection (point_in_view) for view v, all ones without cameras; c = the number of views that see a node.
#define NJF_FUSE_CAM_FLOATS 21  // rows 0..2 of ctxt_w2c + the 9 intrinsics: a CamCtx
static_assert(sizeof(CamCtx) == NJF_FUSE_CAM_FLOATS * sizeof(float), "CamCtx layout");
struct FuseArgs {
  NjfFieldGrid grid;
  int nodes;              // N
  int views;              // V
  int blocks_per_scene;   // ceil(N / NJF_FIELD_SELECT_BLOCK)
  int min_views;
  const float* w2c;       // [G*V,4,4] or null (every view sees every node)
  const float* k;         // [G*V,3,3]
  const float* values;    // [G*V*N]
  float* fused;           // [G*N]
  unsigned char* seen;    // [G*N] or null
  unsigned char* valid;   // [G*N] or null
};

// One workgroup per 1024 consecutive nodes of ONE scene (the item / thread layout of the selection kernels: consecutive
// threads read consecutive floats of every view's values).  The scene's V cameras go to LDS once; views outermost, so a
// thread takes a camera out of LDS once per view and keeps the running state of its four nodes in registers.  fp32 adds in
// view order, one IEEE division, no atomics: the result is a function of the inputs alone.
template <int MODE>
__global__ void __launch_bounds__(NJF_BLOCK_THREADS) field_fuse_kernel(FuseArgs a) {
  __shared__ float cams[NJF_FIELD_MAX_VIEWS * NJF_FUSE_CAM_FLOATS];
  const int g = blockIdx.x / a.blocks_per_scene;
  const int first = (blockIdx.x - g * a.blocks_per_scene) * NJF_FIELD_SELECT_BLOCK;
  if (a.w2c) {
    for (int t = threadIdx.x; t < a.views * NJF_FUSE_CAM_FLOATS; t += NJF_BLOCK_THREADS) {
      const int v = t / NJF_FUSE_CAM_FLOATS, e = t - v * NJF_FUSE_CAM_FLOATS;
      const size_t b = (size_t)g * a.views + v;
      cams[t] = e < 12 ? a.w2c[b * 16 + e] : a.k[b * 9 + (e - 12)];
    }
    __syncthreads();
  }
  float px[NJF_BLOCK_ITEMS], py[NJF_BLOCK_ITEMS], pz[NJF_BLOCK_ITEMS], acc[NJF_BLOCK_ITEMS];
  int count[NJF_BLOCK_ITEMS];
  unsigned mask[NJF_BLOCK_ITEMS];
  const int yz = a.grid.dims[1] * a.grid.dims[2];
#pragma unroll
  for (int it = 0; it < NJF_BLOCK_ITEMS; ++it) {
    const int n = min(first + it * NJF_BLOCK_THREADS + (int)threadIdx.x, a.nodes - 1);  // (the node of field_node)
    const int ix = n / yz, r = n - ix * yz;
    const int iy = r / a.grid.dims[2], iz = r - iy * a.grid.dims[2];
    px[it] = fmaf((float)ix, a.grid.step[0], a.grid.origin[0]);
    py[it] = fmaf((float)iy, a.grid.step[1], a.grid.origin[1]);
    pz[it] = fmaf((float)iz, a.grid.step[2], a.grid.origin[2]);
    acc[it] = 0.0f;
    count[it] = 0;
    mask[it] = 0u;
  }
  for (int v = 0; v < a.views; ++v) {
    CamCtx cam;
    if (a.w2c) {
#pragma unroll
      for (int i = 0; i < 12; ++i) cam.m[i] = cams[v * NJF_FUSE_CAM_FLOATS + i];
#pragma unroll
      for (int i = 0; i < 9; ++i) cam.k[i] = cams[v * NJF_FUSE_CAM_FLOATS + 12 + i];
    }
    const float* __restrict__ row = a.values + ((size_t)g * a.views + v) * (size_t)a.nodes;
#pragma unroll
    for (int it = 0; it < NJF_BLOCK_ITEMS; ++it) {
      const int n = first + it * NJF_BLOCK_THREADS + (int)threadIdx.x;
      if (n >= a.nodes) continue;
      if (a.w2c && !point_in_view(cam, px[it], py[it], pz[it])) continue;
      const float d = row[n];
      if (MODE == NJF_FIELD_FUSE_MEAN) acc[it] += d;
      else if (count[it] == 0) acc[it] = d;
      else if (MODE == NJF_FIELD_FUSE_MIN) acc[it] = (d < acc[it]) ? d : acc[it];
      else acc[it] = (d > acc[it]) ? d : acc[it];
      ++count[it];
      mask[it] |= 1u << v;
    }
  }
#pragma unroll
  for (int it = 0; it < NJF_BLOCK_ITEMS; ++it) {
    const int n = first + it * NJF_BLOCK_THREADS + (int)threadIdx.x;
    if (n >= a.nodes) continue;
    const bool ok = count[it] >= a.min_views;
    float f = acc[it];
    if (MODE == NJF_FIELD_FUSE_MEAN) f = f / (float)count[it];
    const size_t o = (size_t)g * a.nodes + n;
    a.fused[o] = ok ? f : 0.0f;
    if (a.seen) a.seen[o] = (unsigned char)mask[it];
    if (a.valid) a.valid[o] = ok ? 1 : 0;
  }
}

// Colour and Jacobian at the positions of a list (survivor nodes or mesh vertices) from the per-view rows of the decoder:
// w_v = s_v(x) ? d_v(x) : 0, W = the sum of the w_v (fp32 adds, v ascending), every w_v = 1 and W = V if not W > 0,
// out = (fma chain over v) / W.  Per-view rows are entry-major: row i*V + v.
#define NJF_COMBINE_THREADS 256
struct CombineArgs {
  const float* xyz;        // [capacity, 3]
  const int* node;         // [capacity] fused global index: the scene of entry i is node[i] / nodes
  const int* count;        // or null
  int capacity;
  int nodes, scenes;       // N, G (scenes: only with cameras)
  int views;
  const float* w2c;        // [G*V,4,4] or null
  const float* k;
  const float* density;    // [capacity*V] (null: nothing to weigh, `views` alone is written)
  const float* color;      // [capacity*V, 3] or null
  const float* jacobian;   // [capacity*V, 3A] or null
  int jdim;                // 3A
  float* out_color;        // [capacity, 3]
  float* out_jacobian;     // [capacity, 3A]
  unsigned char* out_views;  // [capacity] or null
};

// out[i, c] for the workgroup's entries: consecutive threads take consecutive floats of the output (and of every view's
// input row, which is contiguous per entry)
__device__ __forceinline__ void combine_rows(const float* __restrict__ in, float* __restrict__ out, int dim, int first, int rows,
                                             int views, const float (*w)[NJF_COMBINE_THREADS], const float* wsum) {
  for (int e = threadIdx.x; e < rows * dim; e += NJF_COMBINE_THREADS) {
    const int il = e / dim, c = e - il * dim;
    const size_t i = (size_t)first + il;
    float acc = 0.0f;
    for (int v = 0; v < views; ++v) acc = fmaf(w[v][il], in[(i * views + v) * dim + c], acc);
    out[i * dim + c] = acc / wsum[il];
  }
}

__global__ void __launch_bounds__(NJF_COMBINE_THREADS) field_combine_kernel(CombineArgs a) {
  __shared__ float w[NJF_FIELD_MAX_VIEWS][NJF_COMBINE_THREADS];
  __shared__ float wsum[NJF_COMBINE_THREADS];
  const int entries = counted_length(a.count, a.capacity);
  const int first = blockIdx.x * NJF_COMBINE_THREADS;
  if (first >= entries) return;  // the whole workgroup, before any barrier
  const int rows = min(NJF_COMBINE_THREADS, entries - first);
  const int il = threadIdx.x;
  if (il < rows) {
    const size_t i = (size_t)first + il;
    unsigned mask = (1u << a.views) - 1u;
    if (a.w2c) {
      const int g = min(max(a.node[i], 0) / a.nodes, a.scenes - 1);  // (caller data: clamped into the scenes)
      const float px = a.xyz[3 * i], py = a.xyz[3 * i + 1], pz = a.xyz[3 * i + 2];
      mask = 0u;
      for (int v = 0; v < a.views; ++v) {
        CamCtx cam;
        load_ctx(a.w2c, a.k, g * a.views + v, cam);
        mask |= point_in_view(cam, px, py, pz) ? 1u << v : 0u;
      }
    }
    if (a.out_views) a.out_views[i] = (unsigned char)mask;
    if (a.density) {
      float total = 0.0f;
      for (int v = 0; v < a.views; ++v) {
        const float wv = ((mask >> v) & 1u) ? a.density[i * a.views + v] : 0.0f;
        w[v][il] = wv;
        total += wv;
      }
      if (!(total > 0.0f)) {  // no view sees the position, or every density is zero (or NaN): the plain mean
        for (int v = 0; v < a.views; ++v) w[v][il] = 1.0f;
        total = (float)a.views;
      }
      wsum[il] = total;
    }
  }
  if (!a.density) return;
  __syncthreads();
  if (a.color) combine_rows(a.color, a.out_color, 3, first, rows, a.views, w, wsum);
  if (a.jacobian) combine_rows(a.jacobian, a.out_jacobian, a.jdim, first, rows, a.views, w, wsum);
}

// ---- connected components of the inside nodes: lock-free union-find ---------------------------------------------------------
// inside(g) = valid(g) && values[g] >= threshold (NaN: outside; valid = the caller's mask and / or point_in_view), or -- list
// form -- g is an entry of an ascending index list.  Two inside nodes of one batch element are adjacent iff they differ by one
// of the first `half` = C/2 directions of the mesh table (3: the axes; 7: the edges of the Kuhn tetrahedra), in either sign,
// and -- with keys -- carry equal keys.  labels[g] = the smallest global index of g's component (-1 outside), sizes[g] = its
// node count (0 outside), *count = the number of components.
// parent[g] (int32, -1 outside) is a forest with the invariant parent[g] <= g AT ALL TIMES: launch 1 writes the minimum of the
// in-workgroup component, every later write is an atomicMin with a smaller index of the same final component.  Hence every
// chain strictly decreases and ends at a root (parent[r] == r), roots only ever move to smaller indices, and the final root
// of a tree is the minimum of its component.  Four launches over workgroups of 1024 consecutive nodes, item-major:
//   1 components_init_kernel   inside flags, in-workgroup unions in LDS, parent / per-local-root counts / zeros to memory
//   2 components_merge_kernel  unions of the adjacent pairs whose ends lie in different workgroups
//   3 components_label_kernel  labels = find, one atomicAdd per LOCAL ROOT into root_size[label], the component count
//   4 components_size_kernel   sizes = root_size[labels]
// Memory rules of launch 2 (the XCDs' L2s are not coherent for plain accesses inside a launch): every write to parent is an
// agent-scope atomicMin, every read of it a relaxed agent-scope atomic load, and no decision rests on the freshness of a
// load: a stale parent is an older link of the same final component (it costs a retry), and a union only ends on the value
// an atomicMin RETURNED.  Launches 3 and 4 read what earlier launches wrote: plain loads.
#define NJF_CC_THREADS 256
#define NJF_CC_ITEMS (NJF_FIELD_COMPONENTS_BLOCK / NJF_CC_THREADS)
#define NJF_CC_WAVES (NJF_CC_THREADS / 64)
#define NJF_CC_FIND_CAP (1 << 20)   // hops of one find: a chain strictly decreases, so B*N bounds it; past this, status
#define NJF_CC_UNION_CAP (1 << 12)  // retries of one union: each needs another workgroup's link to land in between
static_assert(NJF_CC_ITEMS * NJF_CC_THREADS == NJF_FIELD_COMPONENTS_BLOCK && NJF_FIELD_COMPONENTS_BLOCK == NJF_FIELD_MESH_BLOCK,
              "components block");
struct ComponentArgs {
  SelectArgs sel;              // list: the identity over B*N; values, threshold; w2c / k: frustum part of `valid` (or null)
  const unsigned char* valid;  // [B*N] or null
  const int* entries;          // list form: ascending global indices (null: the dense form)
  const int* entry_count;      // device count of the list or null
  int entry_capacity;
  const int* keys;             // dense form: [B*N]; list form: [entry_capacity], per entry; or null
  int* dense_keys;             // [B*N]: what launch 2 reads (dense form: == keys; list form: scattered by launch 1)
  int half;                    // C / 2 directions
  int* parent;                 // [B*N]
  int* root_size;              // [B*N]
  int* labels;                 // [B*N]
  int* sizes;                  // [B*N]: launches 1..3 keep the node count of every local root here (0 elsewhere)
  int* count;
  int* status;
};

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int cc_load_lds(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// (ix, iy, iz) of global index gi
__device__ __forceinline__ void cc_coords(const FieldList& l, int gi, int& ix, int& iy, int& iz) {
  const int n = gi % l.nodes;
  const int yz = l.grid.dims[1] * l.grid.dims[2];
  ix = n / yz;
  const int r = n - ix * yz;
  iy = r / l.grid.dims[2];
  iz = r - iy * l.grid.dims[2];
}

// does the neighbour of (ix, iy, iz) in direction `code` exist in the grid (no wrap at the faces)?
__device__ __forceinline__ bool cc_in_grid(const NjfFieldGrid& g, int ix, int iy, int iz, int code) {
  return ix + (code & 1) < g.dims[0] && iy + ((code >> 1) & 1) < g.dims[1] && iz + (code >> 2) < g.dims[2];
}

// Root of x in the LDS forest of one workgroup (lab[y] <= y: a chain strictly decreases inside [0, 1024), so it has at most
// 1023 hops; the cap can only trip on a broken invariant).
__device__ __forceinline__ int cc_find_lds(const int* lab, int x, int* status) {
  for (int hop = 0; hop < NJF_FIELD_COMPONENTS_BLOCK; ++hop) {
    const int p = cc_load_lds(lab + x);
    if (p == x || p < 0) return x;
    x = p;
  }
  atomicOr(status, NJF_FIELD_COMPONENTS_E_LOCAL);
  return x;
}

// Union in LDS.  Terminates: a retry happens only when the atomicMin found that another thread had lowered lab[a] in
// between, and it continues from that strictly smaller index, so a + b strictly decreases from retry to retry.
__device__ __forceinline__ void cc_union_lds(int* lab, int a, int b, int* status) {
  for (int t = 0; t < NJF_FIELD_COMPONENTS_BLOCK; ++t) {
    a = cc_find_lds(lab, a, status);
    b = cc_find_lds(lab, b, status);
    if (a == b) return;
    if (a < b) { const int s = a; a = b; b = s; }
    const int old = atomicMin(lab + a, b);
    if (old == a) return;  // a WAS a root (the atomic says so) and now hangs under b
    a = old;               // a already hung under old < a: old and b still have to meet
  }
  atomicOr(status, NJF_FIELD_COMPONENTS_E_LOCAL);
}

// Root of x in the global forest, launch 2.  Terminates: every value ever stored in parent[y] is <= y, fresh or stale, so the
// chain strictly decreases; it ends at an index that (as far as this load could see) is a root.  A stale answer is a node of
// the same final component that has since been linked further: the caller's atomicMin finds that out.  The start of the
// chain is then hooked to what was found (an atomicMin with a smaller index of its own component: the invariant holds).
__device__ __forceinline__ int cc_find(int* parent, int x, int* status) {
  const int x0 = x;
  int first = -1;
  for (int hop = 0; hop < NJF_CC_FIND_CAP; ++hop) {
    const int p = cc_load(parent + x);
    if (hop == 0) first = p;
    if (p == x || p < 0) {
      if (first != x && x < x0) atomicMin(parent + x0, x);
      return x;
    }
    x = p;
  }
  atomicOr(status, NJF_FIELD_COMPONENTS_E_FIND);
  return x;
}

// union(a, b), launch 2: find both roots, atomicMin(&parent[larger], smaller), and continue from the returned value if the
// larger one was no longer a root.  The only exits are a == b (one node: nothing to join) and an atomicMin that returned its
// own address' index (it WAS a root when the link landed).  Terminates: a retry continues from old < a with b unchanged, and
// a find only lowers its argument, so a + b strictly decreases from retry to retry; every retry is caused by a link of
// another thread that landed in between.
__device__ __forceinline__ void cc_union(int* parent, int a, int b, int* status) {
  for (int t = 0; t < NJF_CC_UNION_CAP; ++t) {
    a = cc_find(parent, a, status);
    b = cc_find(parent, b, status);
    if (a == b) return;
    if (a < b) { const int s = a; a = b; b = s; }
    const int old = atomicMin(parent + a, b);
    if (old == a) return;
    a = old;
  }
  atomicOr(status, NJF_FIELD_COMPONENTS_E_UNION);
}

// first list position whose entry is >= key (the list is ascending)
__device__ __forceinline__ int cc_lower_bound(const int* list, int n, long long key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((long long)list[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// launch 1
template <bool LIST>
__global__ void __launch_bounds__(NJF_CC_THREADS) components_init_kernel(ComponentArgs a) {
  __shared__ int lab[NJF_FIELD_COMPONENTS_BLOCK];   // local parent (index inside the workgroup), -1 outside
  __shared__ int cnt[NJF_FIELD_COMPONENTS_BLOCK];   // nodes per local root
  __shared__ int keyl[NJF_FIELD_COMPONENTS_BLOCK];
  __shared__ int range[2];
  const FieldList& fl = a.sel.list;
  const long long base = (long long)blockIdx.x * NJF_FIELD_COMPONENTS_BLOCK;
  const int nloc = (int)min((long long)NJF_FIELD_COMPONENTS_BLOCK, (long long)fl.total - base);
  const int tid = threadIdx.x;
#pragma unroll
  for (int it = 0; it < NJF_CC_ITEMS; ++it) {
    const int l = it * NJF_CC_THREADS + tid;
    cnt[l] = 0;
    keyl[l] = 0;
    if (LIST) {
      lab[l] = -1;
    } else {
      bool in = l < nloc;
      const int gi = (int)(base + min(l, nloc - 1));
      if (in) in = a.sel.values[gi] >= a.sel.threshold;
      if (in && a.valid) in = a.valid[gi] != 0;
      if (in && a.sel.w2c) in = field_in_view(a.sel, gi);
      lab[l] = in ? l : -1;
      if (in && a.keys) keyl[l] = a.keys[gi];
    }
  }
  if (LIST) {
    const int n = counted_length(a.entry_count, a.entry_capacity);
    if (tid < 2) range[tid] = cc_lower_bound(a.entries, n, base + (tid ? nloc : 0));
    __syncthreads();
    for (int e = range[0] + tid; e < range[1]; e += NJF_CC_THREADS) {
      const long long l = (long long)a.entries[e] - base;
      if (l < 0 || l >= nloc) continue;   // (caller data: an unsorted list loses entries, it never addresses outside)
      lab[l] = (int)l;
      if (a.keys) keyl[l] = a.keys[e];
    }
  }
  __syncthreads();
  // unions of the pairs with both ends in this workgroup (the upper end lies `off` entries further on)
#pragma unroll
  for (int it = 0; it < NJF_CC_ITEMS; ++it) {
    const int l = it * NJF_CC_THREADS + tid;
    if (l >= nloc || cc_load_lds(lab + l) < 0) continue;
    int ix, iy, iz;
    cc_coords(fl, (int)(base + l), ix, iy, iz);
    for (int k = 0; k < a.half; ++k) {
      const int code = mesh_dir_code(k);
      if (!cc_in_grid(fl.grid, ix, iy, iz, code)) continue;
      const int l1 = l + mesh_code_offset(fl.grid, code);
      if (l1 >= nloc || cc_load_lds(lab + l1) < 0 || keyl[l1] != keyl[l]) continue;
      cc_union_lds(lab, l, l1, a.status);
    }
  }
  __syncthreads();
  int root[NJF_CC_ITEMS];
#pragma unroll
  for (int it = 0; it < NJF_CC_ITEMS; ++it) {
    const int l = it * NJF_CC_THREADS + tid;
    root[it] = (l < nloc && lab[l] >= 0) ? cc_find_lds(lab, l, a.status) : -1;
    // one LDS add per wave where the wave's inside nodes share a root (the inside of a large body), else one per node
    const bool in = root[it] >= 0;
    const unsigned long long m = __ballot(in);
    if (m == 0ull) continue;  // (wave-uniform)
    const int lead = __ffsll((long long)m) - 1;
    const int r0 = __shfl(root[it], lead, 64);
    if (__all(!in || root[it] == r0)) {
      if ((tid & 63) == lead) atomicAdd(cnt + r0, __popcll(m));
    } else if (in) {
      atomicAdd(cnt + root[it], 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < NJF_CC_ITEMS; ++it) {
    const int l = it * NJF_CC_THREADS + tid;
    if (l >= nloc) continue;
    const int gi = (int)(base + l);
    a.parent[gi] = root[it] >= 0 ? (int)base + root[it] : -1;
    a.sizes[gi] = root[it] == l ? cnt[l] : 0;
    a.root_size[gi] = 0;
    if (LIST && a.keys) a.dense_keys[gi] = keyl[l];
  }
}

// launch 2
__global__ void __launch_bounds__(NJF_CC_THREADS) components_merge_kernel(ComponentArgs a) {
  const FieldList& fl = a.sel.list;
  const long long base = (long long)blockIdx.x * NJF_FIELD_COMPONENTS_BLOCK;
  const int nloc = (int)min((long long)NJF_FIELD_COMPONENTS_BLOCK, (long long)fl.total - base);
#pragma unroll
  for (int it = 0; it < NJF_CC_ITEMS; ++it) {
    const int l = it * NJF_CC_THREADS + (int)threadIdx.x;
    if (l >= nloc) continue;
    const int gi = (int)(base + l);
    if (cc_load(a.parent + gi) < 0) continue;   // (-1 is written by launch 1 alone and never changes)
    int ix, iy, iz;
    cc_coords(fl, gi, ix, iy, iz);
    for (int k = 0; k < a.half; ++k) {
      const int code = mesh_dir_code(k);
      if (!cc_in_grid(fl.grid, ix, iy, iz, code)) continue;
      const int off = mesh_code_offset(fl.grid, code);
      if (l + off < nloc) continue;             // both ends in this workgroup: launch 1 joined them
      const int g1 = gi + off;                  // (inside the batch element's grid, hence below B*N)
      if (cc_load(a.parent + g1) < 0) continue;
      if (a.dense_keys && a.dense_keys[g1] != a.dense_keys[gi]) continue;
      cc_union(a.parent, gi, g1, a.status);
    }
  }
}

// launch 3 (parent is final: plain loads of what launches 1 and 2 wrote)
__global__ void __launch_bounds__(NJF_CC_THREADS) components_label_kernel(ComponentArgs a) {
  __shared__ int wave_part[NJF_CC_WAVES];
  const FieldList& fl = a.sel.list;
  const long long base = (long long)blockIdx.x * NJF_FIELD_COMPONENTS_BLOCK;
  const int nloc = (int)min((long long)NJF_FIELD_COMPONENTS_BLOCK, (long long)fl.total - base);
  int roots = 0;
#pragma unroll
  for (int it = 0; it < NJF_CC_ITEMS; ++it) {
    const int l = it * NJF_CC_THREADS + (int)threadIdx.x;
    if (l >= nloc) continue;
    const int gi = (int)(base + l);
    int x = gi, p = a.parent[gi];
    if (p < 0) {
      a.labels[gi] = -1;
      continue;
    }
    // the chain strictly decreases (parent[y] <= y) and nothing writes parent any more: at most B*N hops
    int hop = 0;
    for (; p != x && p >= 0 && hop < NJF_CC_FIND_CAP; ++hop) {
      x = p;
      p = a.parent[x];
    }
    if (hop == NJF_CC_FIND_CAP) atomicOr(a.status, NJF_FIELD_COMPONENTS_E_FIND);
    a.labels[gi] = x;
    roots += x == gi;
    const int c = a.sizes[gi];              // > 0 at the local roots of launch 1 only
    if (c > 0) atomicAdd(a.root_size + x, c);
  }
  const int s = block_sum(roots, wave_part);
  if (threadIdx.x == 0 && s > 0) atomicAdd(a.count, s);
}

// launch 4
__global__ void __launch_bounds__(NJF_CC_THREADS) components_size_kernel(ComponentArgs a) {
  const FieldList& fl = a.sel.list;
  const long long base = (long long)blockIdx.x * NJF_FIELD_COMPONENTS_BLOCK;
  const int nloc = (int)min((long long)NJF_FIELD_COMPONENTS_BLOCK, (long long)fl.total - base);
#pragma unroll
  for (int it = 0; it < NJF_CC_ITEMS; ++it) {
    const int l = it * NJF_CC_THREADS + (int)threadIdx.x;
    if (l >= nloc) continue;
    const int gi = (int)(base + l);
    const int r = a.labels[gi];
    a.sizes[gi] = r >= 0 ? a.root_size[r] : 0;
  }
}

// ---- coarse-to-fine band: the fine density pass only near the surface --------------------------------
// The fine grid (nx, ny, nz) with (n_c - 1) % k == 0 is cut into BLOCKS of k^3 cells: m_c = (n_c - 1) / k per axis, block
// (jx, jy, jz) has the local index (jx*m_y + jy)*m_z + jz.  Coarse node j IS fine node k*j (k is a power of two, so k*step is
// exact), M = prod(m_c + 1) per element.  hit(b, q) = (coarse_valid == null || coarse_valid[b, q]) && coarse_values[b, q] >=
// threshold (NaN: no hit); block j is ACTIVE iff a coarse node q with max(0, j_c - d) <= q_c <= min(m_c, j_c + 1 + d) on every
// axis is a hit; fine node i is in the BAND iff an active block j has j_c*k <= i_c <= (j_c + 1)*k on every axis -- the
// candidates per axis are {ceil(i_c / k) - 1, floor(i_c / k)} clipped to [0, m_c - 1].  Workgroups of 1024 consecutive nodes
// on the workgroup primitives, like the selection; the one atomic is an integer add per workgroup of the leak count.
struct BandArgs {
  int dims[3];                   // fine grid
  int nodes, total;              // N, B*N
  int batch;
  int shift;                     // log2 k
  int m[3];                      // blocks per axis
  int nb;                        // Nb = m_x*m_y*m_z
  int dilate;
  const float* cvalues;          // [B, M]
  const unsigned char* cvalid;   // [B, M] or null
  float cthreshold;
  unsigned char* block_active;   // [B*Nb]
  unsigned char* band;           // [B*N]
  int* out_indices;
  int* out_count;
  int out_capacity;
  int* block_counts;             // [ceil(B*N / 1024)]: counts, then (after the scan) exclusive offsets
};

// one thread per block: any hit among its (2d + 2)^3 clipped coarse nodes
__global__ void __launch_bounds__(NJF_BLOCK_THREADS) band_blocks_kernel(BandArgs a) {
  const int g = blockIdx.x * NJF_BLOCK_THREADS + threadIdx.x;
  if (g >= a.batch * a.nb) return;
  const int b = g / a.nb, j = g - b * a.nb;
  const int myz = a.m[1] * a.m[2];
  const int jx = j / myz, r = j - jx * myz;
  const int jy = r / a.m[2], jz = r - jy * a.m[2];
  const int cy = a.m[1] + 1, cz = a.m[2] + 1;
  const size_t cbase = (size_t)b * (size_t)(a.m[0] + 1) * (size_t)(cy * cz);
  const int d = a.dilate;
  const int x0 = max(0, jx - d), x1 = min(a.m[0], jx + 1 + d);
  const int y0 = max(0, jy - d), y1 = min(a.m[1], jy + 1 + d);
  const int z0 = max(0, jz - d), z1 = min(a.m[2], jz + 1 + d);
  bool hit = false;
  for (int qx = x0; qx <= x1; ++qx)
    for (int qy = y0; qy <= y1; ++qy)
      for (int qz = z0; qz <= z1; ++qz) {
        const size_t q = cbase + (size_t)((qx * cy + qy) * cz + qz);
        hit |= (!a.cvalid || a.cvalid[q] != 0) && a.cvalues[q] >= a.cthreshold;  // (NaN compares false)
      }
  a.block_active[g] = hit ? 1 : 0;
}

// is node gi (a global index below B*N) inside an active block of its element?  At most eight block bytes.
__device__ __forceinline__ bool band_node(const BandArgs& a, int gi) {
  const int b = gi / a.nodes, n = gi - b * a.nodes;
  const int yz = a.dims[1] * a.dims[2];
  const int ix = n / yz, r = n - ix * yz;
  const int iy = r / a.dims[2], iz = r - iy * a.dims[2];
  const int round_up = (1 << a.shift) - 1;
  const int x0 = max(((ix + round_up) >> a.shift) - 1, 0), x1 = min(ix >> a.shift, a.m[0] - 1);
  const int y0 = max(((iy + round_up) >> a.shift) - 1, 0), y1 = min(iy >> a.shift, a.m[1] - 1);
  const int z0 = max(((iz + round_up) >> a.shift) - 1, 0), z1 = min(iz >> a.shift, a.m[2] - 1);
  const unsigned char* act = a.block_active + (size_t)b * (size_t)a.nb;
  bool in = false;
  for (int jx = x0; jx <= x1; ++jx)
    for (int jy = y0; jy <= y1; ++jy)
      for (int jz = z0; jz <= z1; ++jz) in |= act[(jx * a.m[1] + jy) * a.m[2] + jz] != 0;
  return in;
}

// band bytes + per-workgroup counts
__global__ void __launch_bounds__(NJF_BLOCK_THREADS) band_count_kernel(BandArgs a) {
  __shared__ int wave_count[NJF_BLOCK_WAVES];
  int n = 0;
#pragma unroll
  for (int it = 0; it < NJF_BLOCK_ITEMS; ++it) {
    const long long i = (long long)blockIdx.x * NJF_FIELD_BAND_BLOCK + it * NJF_BLOCK_THREADS + threadIdx.x;
    bool in = false;
    if (i < a.total) {
      in = band_node(a, (int)i);
      a.band[i] = in ? 1 : 0;
    }
    n += __popcll(__ballot(in));  // wave-uniform
  }
  const int s = block_sum_waves(n, wave_count);
  if (threadIdx.x == 0) a.block_counts[blockIdx.x] = s;
}

// the ascending global indices of the band nodes (the band bytes and the scanned offsets come from earlier launches)
__global__ void __launch_bounds__(NJF_BLOCK_THREADS) band_scatter_kernel(BandArgs a) {
  __shared__ int wave_count[NJF_BLOCK_ITEMS][NJF_BLOCK_WAVES];
  unsigned flags = 0;
#pragma unroll
  for (int it = 0; it < NJF_BLOCK_ITEMS; ++it) {
    const long long i = (long long)blockIdx.x * NJF_FIELD_BAND_BLOCK + it * NJF_BLOCK_THREADS + threadIdx.x;
    flags |= i < a.total && a.band[i] != 0 ? 1u << it : 0u;
  }
  block_flag_ranks(flags, a.block_counts[blockIdx.x], wave_count, [&](int it, int rank) {
    if (rank < a.out_capacity) a.out_indices[rank] = blockIdx.x * NJF_FIELD_BAND_BLOCK + it * NJF_BLOCK_THREADS + threadIdx.x;
  });
}

// out[indices[i]] = values[i] for i < min(*count, capacity); an index outside [0, out_size) is skipped
__global__ void __launch_bounds__(256) field_scatter_kernel(const float* __restrict__ values, const int* __restrict__ indices,
                                                            const int* __restrict__ count, int capacity, float* __restrict__ out,
                                                            int out_size) {
  const int entries = counted_length(count, capacity);
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= entries) return;  // (a workgroup past the count leaves; rows past the count are never read)
  const int g = indices[i];
  if (g >= 0 && g < out_size) out[g] = values[i];
}

struct BandLeakArgs {
  int dims[3];
  int nodes, total;
  const unsigned char* band;  // [B*N]
  const int* indices;         // the inside nodes, ascending global indices
  const int* count;           // or null
  int capacity;
  int* leaks;
};

// entries with a neighbour g +- dir_k (the seven mesh directions, inside the grid: no wrap at the faces) outside the band
__global__ void __launch_bounds__(NJF_BLOCK_THREADS) band_leaks_kernel(BandLeakArgs a) {
  __shared__ int wave_count[NJF_BLOCK_WAVES];
  const int entries = counted_length(a.count, a.capacity);
  const long long base = (long long)blockIdx.x * NJF_FIELD_BAND_BLOCK;
  if (base >= entries) return;  // (uniform over the workgroup)
  int n = 0;
#pragma unroll
  for (int it = 0; it < NJF_BLOCK_ITEMS; ++it) {
    const long long i = base + it * NJF_BLOCK_THREADS + threadIdx.x;
    bool leak = false;
    if (i < entries) {
      const int g = a.indices[i];
      if (g >= 0 && g < a.total) {
        const int node = g % a.nodes;
        const int yz = a.dims[1] * a.dims[2];
        const int ix = node / yz, r = node - ix * yz;
        const int iy = r / a.dims[2], iz = r - iy * a.dims[2];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
          // direction k of the mesh table: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1)
          const int dx = (0x59 >> k) & 1, dy = (0x6a >> k) & 1, dz = (0x74 >> k) & 1;
          const int off = (dx * a.dims[1] + dy) * a.dims[2] + dz;
          const bool up = ix + dx < a.dims[0] && iy + dy < a.dims[1] && iz + dz < a.dims[2];
          const bool down = ix - dx >= 0 && iy - dy >= 0 && iz - dz >= 0;
          if (up) leak |= a.band[g + off] == 0;
          if (down) leak |= a.band[g - off] == 0;
        }
      }
    }
    n += __popcll(__ballot(leak));
  }
  const int s = block_sum_waves(n, wave_count);
  if (threadIdx.x == 0 && s) atomicAdd(a.leaks, s);  // one integer add per workgroup: the sum does not depend on the order
}

// =============================================================================================
// rigid twists per part and command channel (njf_field_twists)
// =============================================================================================
// J_a(x) = v_a + omega_a x (x - c) fitted per part (the rows of one label) and channel, in double, without floating-point atomics:
// workgroup (chunk, part) compacts the chunk's matching rows IN ORDER into LDS (block_flag_ranks), thread t accumulates list
// entries t, t + 256, ... sequentially, the butterfly (wave_sum) and the four wave partials in wave order give partial[part][chunk][.], and a finishing
// kernel adds the chunks in ascending order.  Every sum therefore has an order that depends on (n, K, A) alone.
#define NJF_TWIST_THREADS 256
#define NJF_TWIST_ITEMS (NJF_FIELD_TWISTS_CHUNK / NJF_TWIST_THREADS)
#define NJF_TWIST_MAX_VALUES NJF_FIELD_TWISTS_STRIDE(NJF_MAX_ACTION_DIM)
struct TwistArgs {
  const float* xyz;       // [n,3]
  const float* jac;       // [n,A,3]
  const int* labels;      // [n]
  const float* weights;   // [n] or null
  const int* count;       // or null
  int n, A;
  const int* parts;       // [K]
  const int* parts_count; // or null
  int K, chunks, stride;
  int *out_labels, *out_count, *nodes, *status;
  double *weight, *centroid, *omega, *velocity, *energy, *residual, *q, *p, *l;
  float* row_residual;
  double* partial;        // [K][chunks][stride]
};

__device__ __forceinline__ int twist_active(const TwistArgs& a) { return counted_length(a.parts_count, a.K); }
__device__ __forceinline__ int twist_rows(const TwistArgs& a) { return counted_length(a.count, a.n); }
__device__ __forceinline__ double twist_weight(const TwistArgs& a, long long i) {
  if (!a.weights) return 1.0;
  const float w = a.weights[i];
  return w > 0.f ? (double)w : 0.0;  // (NaN and negatives count as 0)
}

// the chunk's rows of label `part`, as offsets into the chunk, ascending, into list[]; returns their number
// (block_flag_ranks from 0: the ranks are the places in the list; the workgroup size comes with wave_count)
template <int ITEMS, int WAVES>
__device__ __forceinline__ int twist_compact(const int* labels, int part, int rows, int* list, int (&wave_count)[ITEMS][WAVES]) {
  static_assert(ITEMS * WAVES * 64 == NJF_FIELD_TWISTS_CHUNK && ITEMS <= 32, "a chunk per workgroup");
  const long long base = (long long)blockIdx.x * NJF_FIELD_TWISTS_CHUNK;
  unsigned flags = 0;
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    const long long i = base + it * (WAVES * 64) + threadIdx.x;
    if (i < rows && labels[i] == part) flags |= 1u << it;
  }
  const int m = block_flag_ranks(flags, 0, wave_count, [&](int it, int rank) { list[rank] = it * (WAVES * 64) + threadIdx.x; });
  __syncthreads();
  return m;
}

// pass A: nodes, W = sum w, S = sum w x
__global__ void __launch_bounds__(NJF_TWIST_THREADS) twist_sums_kernel(TwistArgs a) {
  __shared__ int list[NJF_FIELD_TWISTS_CHUNK];
  __shared__ int wave_count[NJF_TWIST_ITEMS][NJF_TWIST_THREADS / 64];
  __shared__ double red[NJF_TWIST_THREADS / 64][4];
  const int p = blockIdx.y, tid = threadIdx.x;
  if (p >= twist_active(a)) return;  // (uniform over the workgroup)
  const int m = twist_compact(a.labels, a.parts[p], twist_rows(a), list, wave_count);
  const long long base = (long long)blockIdx.x * NJF_FIELD_TWISTS_CHUNK;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int e = tid; e < m; e += NJF_TWIST_THREADS) {
    const long long i = base + list[e];
    const double w = twist_weight(a, i);
    if (w > 0.0) {
      acc[0] += w;
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[1 + c] += w * (double)a.xyz[i * 3 + c];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double s = wave_sum(acc[k]);
    if ((tid & 63) == 0) red[tid >> 6][k] = s;
  }
  __syncthreads();
  double* out = a.partial + ((size_t)p * a.chunks + blockIdx.x) * a.stride;
  if (tid < 4) out[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  if (tid == 4) out[4] = (double)m;
}

// labels, count, nodes, weight, centroid and the empty bit of the status; an unused slot gets label -1 and zeros
__global__ void __launch_bounds__(64) twist_centroid_kernel(TwistArgs a) {
  __shared__ double fin[5];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int active = twist_active(a);
  if (p == 0 && tid == 0) *a.out_count = a.parts_count ? max(*a.parts_count, 0) : a.K;
  if (p >= active) {
    if (tid == 0) {
      a.out_labels[p] = -1;
      a.nodes[p] = 0;
      a.status[p] = 0;
      a.weight[p] = 0.0;
    }
    if (tid < 3) a.centroid[p * 3 + tid] = 0.0;
    return;
  }
  if (tid < 5) {
    double s = 0.0;
    for (int c = 0; c < a.chunks; ++c) s += a.partial[((size_t)p * a.chunks + c) * a.stride + tid];
    fin[tid] = s;
  }
  __syncthreads();
  const bool some = fin[0] > 0.0;
  if (tid == 0) {
    a.out_labels[p] = a.parts[p];
    a.nodes[p] = (int)fin[4];
    a.status[p] = some ? 0 : NJF_FIELD_TWISTS_EMPTY;
    a.weight[p] = some ? fin[0] : 0.0;
  }
  if (tid < 3) a.centroid[p * 3 + tid] = some ? fin[1 + tid] / fin[0] : 0.0;
}

// pass B, r = x - c: Q = sum w r r^T (xx xy xz yy yz zz), per channel P = sum w J, L = sum w (r x J), E = sum w J.J
__global__ void __launch_bounds__(NJF_TWIST_THREADS) twist_moments_kernel(TwistArgs a) {
  __shared__ int list[NJF_FIELD_TWISTS_CHUNK];
  __shared__ int wave_count[NJF_TWIST_ITEMS][NJF_TWIST_THREADS / 64];
  __shared__ double red[NJF_TWIST_THREADS / 64][NJF_TWIST_MAX_VALUES];
  const int p = blockIdx.y, tid = threadIdx.x;
  if (p >= twist_active(a)) return;
  const int m = twist_compact(a.labels, a.parts[p], twist_rows(a), list, wave_count);
  const long long base = (long long)blockIdx.x * NJF_FIELD_TWISTS_CHUNK;
  const double cx = a.centroid[p * 3], cy = a.centroid[p * 3 + 1], cz = a.centroid[p * 3 + 2];
  {
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int e = tid; e < m; e += NJF_TWIST_THREADS) {
      const long long i = base + list[e];
      const double w = twist_weight(a, i);
      if (w > 0.0) {
        const double rx = (double)a.xyz[i * 3] - cx, ry = (double)a.xyz[i * 3 + 1] - cy, rz = (double)a.xyz[i * 3 + 2] - cz;
        acc[0] += w * (rx * rx);
        acc[1] += w * (rx * ry);
        acc[2] += w * (rx * rz);
        acc[3] += w * (ry * ry);
        acc[4] += w * (ry * rz);
        acc[5] += w * (rz * rz);
      }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double s = wave_sum(acc[k]);
      if ((tid & 63) == 0) red[tid >> 6][k] = s;
    }
  }
  for (int ch = 0; ch < a.A; ++ch) {  // one channel at a time: seven accumulators, not 7 A
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int e = tid; e < m; e += NJF_TWIST_THREADS) {
      const long long i = base + list[e];
      const double w = twist_weight(a, i);
      if (w > 0.0) {
        const double rx = (double)a.xyz[i * 3] - cx, ry = (double)a.xyz[i * 3 + 1] - cy, rz = (double)a.xyz[i * 3 + 2] - cz;
        const float* j = a.jac + ((size_t)i * a.A + ch) * 3;
        const double jx = (double)j[0], jy = (double)j[1], jz = (double)j[2];
        acc[0] += w * jx;
        acc[1] += w * jy;
        acc[2] += w * jz;
        acc[3] += w * (ry * jz - rz * jy);
        acc[4] += w * (rz * jx - rx * jz);
        acc[5] += w * (rx * jy - ry * jx);
        acc[6] += w * ((jx * jx + jy * jy) + jz * jz);
      }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const double s = wave_sum(acc[k]);
      if ((tid & 63) == 0) red[tid >> 6][6 + 7 * ch + k] = s;
    }
  }
  __syncthreads();
  double* out = a.partial + ((size_t)p * a.chunks + blockIdx.x) * a.stride;
  if (tid < 6 + 7 * a.A) out[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// M = tr(Q) I - Q, Cholesky in the order x, y, z; false (omega stays 0) when a pivot is <= 1e-9 tr(M) or not a number
__device__ __forceinline__ bool twist_solve3(const double* Q, const double* L, double* om) {
  const double tr = (Q[0] + Q[3]) + Q[5];
  const double mxx = tr - Q[0], myy = tr - Q[3], mzz = tr - Q[5], mxy = -Q[1], mxz = -Q[2], myz = -Q[4];
  const double floor_ = 1e-9 * ((mxx + myy) + mzz);
  if (!(mxx > floor_)) return false;
  const double l11 = sqrt(mxx), l21 = mxy / l11, l31 = mxz / l11;
  const double d2 = myy - l21 * l21;
  if (!(d2 > floor_)) return false;
  const double l22 = sqrt(d2), l32 = (myz - l31 * l21) / l22;
  const double d3 = mzz - (l31 * l31 + l32 * l32);
  if (!(d3 > floor_)) return false;
  const double l33 = sqrt(d3);
  const double y0 = L[0] / l11, y1 = (L[1] - l21 * y0) / l22, y2 = (L[2] - (l31 * y0 + l32 * y1)) / l33;
  om[2] = y2 / l33;
  om[1] = (y1 - l32 * om[2]) / l22;
  om[0] = (y0 - (l21 * om[1] + l31 * om[2])) / l11;
  return true;
}

// the chunks of pass B in ascending order, then per channel v = P / W and omega = M^-1 L
__global__ void __launch_bounds__(128) twist_solve_kernel(TwistArgs a) {
  __shared__ double fin[NJF_TWIST_MAX_VALUES];
  const int p = blockIdx.x, tid = threadIdx.x, A = a.A;
  const bool used = p < twist_active(a);
  if (tid < 6 + 7 * A) {
    double s = 0.0;
    if (used)
      for (int c = 0; c < a.chunks; ++c) s += a.partial[((size_t)p * a.chunks + c) * a.stride + tid];
    fin[tid] = s;
    if (tid < 6) {
      a.q[p * 6 + tid] = s;
    } else {
      const int ch = (tid - 6) / 7, k = (tid - 6) % 7;
      if (k < 3) a.p[(p * A + ch) * 3 + k] = s;
      else if (k < 6) a.l[(p * A + ch) * 3 + k - 3] = s;
      else a.energy[p * A + ch] = s;
    }
  }
  __syncthreads();
  if (tid < A) {
    double om[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
    const double W = a.weight[p];
    if (used && W > 0.0) {
      const double* f = fin + 6 + 7 * tid;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = f[c] / W;
      const bool full = twist_solve3(fin, f + 3, om);
      if (!full) om[0] = om[1] = om[2] = 0.0;
      if (!full && tid == 0) a.status[p] |= NJF_FIELD_TWISTS_TRANSLATION;  // (M is the part's: every channel agrees)
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      a.omega[(p * A + tid) * 3 + c] = om[c];
      a.velocity[(p * A + tid) * 3 + c] = v[c];
    }
  }
}

// pass C: residual[p][a] = sum w |J_a - (v_a + omega_a x r)|^2, summed directly, and the unweighted row_residual
__global__ void __launch_bounds__(NJF_TWIST_THREADS) twist_residual_kernel(TwistArgs a) {
  __shared__ int list[NJF_FIELD_TWISTS_CHUNK];
  __shared__ int wave_count[NJF_TWIST_ITEMS][NJF_TWIST_THREADS / 64];
  __shared__ double red[NJF_TWIST_THREADS / 64][NJF_MAX_ACTION_DIM];
  __shared__ double tw[NJF_MAX_ACTION_DIM][6];
  const int p = blockIdx.y, tid = threadIdx.x, A = a.A;
  if (p >= twist_active(a)) return;
  if (tid < 3 * A) {
    tw[tid / 3][tid % 3] = a.omega[p * A * 3 + tid];
    tw[tid / 3][3 + tid % 3] = a.velocity[p * A * 3 + tid];
  }
  const int m = twist_compact(a.labels, a.parts[p], twist_rows(a), list, wave_count);  // (its barriers publish tw)
  const long long base = (long long)blockIdx.x * NJF_FIELD_TWISTS_CHUNK;
  const double cx = a.centroid[p * 3], cy = a.centroid[p * 3 + 1], cz = a.centroid[p * 3 + 2];
  double acc[NJF_MAX_ACTION_DIM];
#pragma unroll
  for (int ch = 0; ch < NJF_MAX_ACTION_DIM; ++ch) acc[ch] = 0.0;
  for (int e = tid; e < m; e += NJF_TWIST_THREADS) {
    const long long i = base + list[e];
    const double w = twist_weight(a, i);
    const double rx = (double)a.xyz[i * 3] - cx, ry = (double)a.xyz[i * 3 + 1] - cy, rz = (double)a.xyz[i * 3 + 2] - cz;
    double row = 0.0;
#pragma unroll
    for (int ch = 0; ch < NJF_MAX_ACTION_DIM; ++ch) {
      if (ch < A) {
        const float* j = a.jac + ((size_t)i * A + ch) * 3;
        const double dx = (double)j[0] - (tw[ch][3] + (tw[ch][1] * rz - tw[ch][2] * ry));
        const double dy = (double)j[1] - (tw[ch][4] + (tw[ch][2] * rx - tw[ch][0] * rz));
        const double dz = (double)j[2] - (tw[ch][5] + (tw[ch][0] * ry - tw[ch][1] * rx));
        const double t = (dx * dx + dy * dy) + dz * dz;
        row += t;
        if (w > 0.0) acc[ch] += w * t;
      }
    }
    a.row_residual[i] = (float)row;
  }
#pragma unroll
  for (int ch = 0; ch < NJF_MAX_ACTION_DIM; ++ch) {
    if (ch < A) {  // (uniform)
      const double s = wave_sum(acc[ch]);
      if ((tid & 63) == 0) red[tid >> 6][ch] = s;
    }
  }
  __syncthreads();
  double* out = a.partial + ((size_t)p * a.chunks + blockIdx.x) * a.stride;
  if (tid < A) out[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ void __launch_bounds__(64) twist_residual_sum_kernel(TwistArgs a) {
  const int p = blockIdx.x, tid = threadIdx.x;
  if (tid >= a.A) return;
  double s = 0.0;
  if (p < twist_active(a) && a.status[p] != NJF_FIELD_TWISTS_EMPTY)
    for (int c = 0; c < a.chunks; ++c) s += a.partial[((size_t)p * a.chunks + c) * a.stride + tid];
  a.residual[p * a.A + tid] = s;
}

// =============================================================================================
// joints between parts: grid contacts and relative twists (njf_field_joints)
// =============================================================================================
// Two parts TOUCH where a node of one has a node of the other as its neighbour along one of the first C/2 mesh directions.  The
// rows' slots go into a dense int32 volume [B*N] (-1: no slot), every row then looks up its 3 or 7 positive neighbours and adds
// (1, ix + ix', iy + iy', iz + iz') to entry (lo, hi) of a K x K x 4 table of 64-bit integers: integer atomics only, so the
// table is a function of the inputs alone.  One workgroup lists the pairs of at least min_contacts contacts in ascending
// (lo, hi); thread (j, a) forms the anchor -- the contact midpoint -- and the relative twist there, in double.
#define NJF_JOINT_THREADS 256
#define NJF_JOINT_LIST_THREADS 1024
struct JointArgs {
  int dims[3];
  float origin[3], step[3];
  int nodes, total;        // N, B*N
  const int* indices;      // [n] ascending global indices
  const int* labels;       // [n]
  const int* count;        // or null
  int n;
  const int* parts;        // [K]
  const int* parts_count;  // or null
  int K, A, half, min_contacts, J;
  const int* part_status;  // [K]
  const double *centroid, *omega, *velocity;   // [K,3], [K,A,3], [K,A,3]
  int* volume;             // [B*N] slot of the node, -1 without one
  unsigned long long* table;   // [K][K][4]: contacts, sum2 x, y, z
  int *part_a, *part_b, *status, *out_count;   // [J], [J], [J], [1]
  long long* contacts;     // [J]
  double *anchor, *out_omega, *out_velocity;   // [J,3], [J,A,3], [J,A,3]
};

// each row binary-searches its label in parts[0 : min(parts_count, K)] and writes its slot at its node
__global__ void __launch_bounds__(NJF_JOINT_THREADS) joint_slots_kernel(JointArgs a) {
  const int rows = counted_length(a.count, a.n);
  const long long i = (long long)blockIdx.x * NJF_JOINT_THREADS + threadIdx.x;
  if (i >= rows) return;  // (rows past the count are never read)
  const int g = a.indices[i], label = a.labels[i];
  if (g < 0 || g >= a.total || label < 0) return;
  const int active = counted_length(a.parts_count, a.K);
  const int p = cc_lower_bound(a.parts, active, label);
  if (p < active && a.parts[p] == label) a.volume[g] = p;  // g < B*N
}

// One thread per row: the slots of its positive neighbours, 64-bit integer adds into the pair table.  COMBINE: the lanes of a
// wave that hold the same pair in one direction (a flat face: all of them) are added up first -- a leader loop over the wave's
// distinct keys -- and the leader alone touches memory; otherwise every lane adds for itself.  Same table either way.
template <bool COMBINE>
__global__ void __launch_bounds__(NJF_JOINT_THREADS) joint_contacts_kernel(JointArgs a) {
  const int rows = counted_length(a.count, a.n);
  const long long i = (long long)blockIdx.x * NJF_JOINT_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int g = -1, p = -1, ix = 0, iy = 0, iz = 0;
  if (i < rows) {
    g = a.indices[i];
    if (g >= 0 && g < a.total) {
      p = a.volume[g];
      const int node = g % a.nodes;
      const int yz = a.dims[1] * a.dims[2];
      ix = node / yz;
      const int r = node - ix * yz;
      iy = r / a.dims[2];
      iz = r - iy * a.dims[2];
    }
  }
  // (no early return: the shuffles below need every lane of the wave)
  for (int k = 0; k < a.half; ++k) {
    // direction k of the mesh table: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1)
    const int dx = (0x59 >> k) & 1, dy = (0x6a >> k) & 1, dz = (0x74 >> k) & 1;
    int key = -1;
    if (p >= 0 && ix + dx < a.dims[0] && iy + dy < a.dims[1] && iz + dz < a.dims[2]) {
      // the neighbour is inside the grid, hence in the same batch element, hence below B*N
      const int q = a.volume[g + (dx * a.dims[1] + dy) * a.dims[2] + dz];
      if (q >= 0 && q != p) key = min(p, q) * a.K + max(p, q);  // < K*K
    }
    const long long sx = 2ll * ix + dx, sy = 2ll * iy + dy, sz = 2ll * iz + dz;
    if (!COMBINE) {
      if (key >= 0) {
        unsigned long long* e = a.table + (size_t)key * 4;
        atomicAdd(e, 1ull);
        atomicAdd(e + 1, (unsigned long long)sx);
        atomicAdd(e + 2, (unsigned long long)sy);
        atomicAdd(e + 3, (unsigned long long)sz);
      }
    } else {
      unsigned long long pending = __ballot(key >= 0);
      while (pending) {  // (uniform over the wave)
        const int leader = __ffsll((long long)pending) - 1;
        const int k0 = __shfl(key, leader);
        const bool mine = key == k0;
        const unsigned long long same = __ballot(mine);
        long long tx = mine ? sx : 0, ty = mine ? sy : 0, tz = mine ? sz : 0;
        if (same & (same - 1)) {  // more than one lane holds the key
          tx = wave_sum(tx);
          ty = wave_sum(ty);
          tz = wave_sum(tz);
        }
        if (lane == leader) {
          unsigned long long* e = a.table + (size_t)k0 * 4;
          atomicAdd(e, (unsigned long long)__popcll(same));
          atomicAdd(e + 1, (unsigned long long)tx);
          atomicAdd(e + 2, (unsigned long long)ty);
          atomicAdd(e + 3, (unsigned long long)tz);
        }
        pending &= ~same;
      }
    }
  }
}

// One workgroup: the ordered compaction of the K*K table entries with at least min_contacts contacts (entry lo*K + hi ascending
// is (lo, hi) ascending), the true count, and the padding of the rows past it.
__global__ void __launch_bounds__(NJF_JOINT_LIST_THREADS) joint_list_kernel(JointArgs a) {
  __shared__ int wave_count[1][NJF_JOINT_LIST_THREADS / 64];
  const int tid = threadIdx.x;
  const int entries = a.K * a.K;
  int run = 0;
  for (int base = 0; base < entries; base += NJF_JOINT_LIST_THREADS) {
    const int e = base + tid;
    long long c = 0;
    if (e < entries) c = (long long)a.table[(size_t)e * 4];
    const bool keep = c >= (long long)a.min_contacts;  // (min_contacts >= 1: an empty entry never passes)
    run += block_flag_ranks(keep ? 1u : 0u, run, wave_count, [&](int, int j) {
      if (j < a.J) {
        const int lo = e / a.K, hi = e - lo * a.K;
        a.part_a[j] = lo;
        a.part_b[j] = hi;
        a.contacts[j] = c;
        a.status[j] = a.part_status[lo] | a.part_status[hi];
      }
    });
    __syncthreads();
  }
  if (tid == 0) *a.out_count = run;  // (at most K*(K-1)/2 < 2^15)
  for (int j = min(run, a.J) + tid; j < a.J; j += NJF_JOINT_LIST_THREADS) {
    a.part_a[j] = -1;
    a.part_b[j] = -1;
    a.contacts[j] = 0;
    a.status[j] = 0;
  }
}

// thread (j, a): the anchor of joint j and the relative twist of channel a there; zeros for the unused rows
__global__ void __launch_bounds__(NJF_JOINT_THREADS) joint_twists_kernel(JointArgs a) {
  const int t = blockIdx.x * NJF_JOINT_THREADS + threadIdx.x;
  if (t >= a.J * a.A) return;
  const int j = t / a.A, ch = t - j * a.A;
  const int lo = a.part_a[j], hi = a.part_b[j];
  double x[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
  if (lo >= 0) {
    const unsigned long long* e = a.table + ((size_t)lo * a.K + hi) * 4;  // lo, hi < K
    const double twice = 2.0 * (double)(long long)e[0];
    double u[2][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double m = (double)(long long)e[1 + c] / twice;
      x[c] = (double)a.origin[c] + (double)a.step[c] * m;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int part = s ? hi : lo;
      const double* cs = a.centroid + (size_t)part * 3;
      const double* ws = a.omega + ((size_t)part * a.A + ch) * 3;
      const double* vs = a.velocity + ((size_t)part * a.A + ch) * 3;
      const double rx = x[0] - cs[0], ry = x[1] - cs[1], rz = x[2] - cs[2];
      u[s][0] = vs[0] + (ws[1] * rz - ws[2] * ry);
      u[s][1] = vs[1] + (ws[2] * rx - ws[0] * rz);
      u[s][2] = vs[2] + (ws[0] * ry - ws[1] * rx);
#pragma unroll
      for (int c = 0; c < 3; ++c) w[c] = s ? ws[c] - w[c] : ws[c];  // omega_hi - omega_lo
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = u[1][c] - u[0][c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (ch == 0) a.anchor[(size_t)j * 3 + c] = x[c];
    a.out_omega[((size_t)j * a.A + ch) * 3 + c] = w[c];
    a.out_velocity[((size_t)j * a.A + ch) * 3 + c] = v[c];
  }
}

// =============================================================================================
// posing the parts under a command: twist exponentials along the tree (njf_field_pose)
// =============================================================================================
// Thread (m, p) of the links launch turns the twist of slot p under command m -- its own about its centroid, or the relative
// twist of the joint it hangs on about the joint's anchor -- into the rigid motion G = (R, t) in double; thread (m, p) of the
// chain launch multiplies the G of p's ancestors onto it, the root last, over a walk of at most K steps; a thread of the
// points launch owns one row and applies its part's transform for every command of a tile.  No atomics anywhere.
#define NJF_POSE_THREADS 256
#define NJF_POSE_COMMAND_TILE 32
struct PoseArgs {
  const int* parts;        // [K]
  const int* parts_count;  // or null
  int K, A, J, M;
  const int* part_status;  // [K]
  const double *centroid, *omega, *velocity;             // [K,3], [K,A,3], [K,A,3]
  const int *part_a, *part_b, *joints_count;             // [J], [J], [1] or null (part_a null: no tree)
  const double *anchor, *joint_omega, *joint_velocity;   // [J,3], [J,A,3], [J,A,3]
  const int *parent, *joint_of;                          // [K]
  const float* commands;   // [M,A]
  double* link;            // [M,K,12]: R row-major, then t
  int* link_bits;          // [K]
  double *rotation, *translation;   // [M,K,9], [M,K,3]
  int *status, *depth;     // [K]
  const float* xyz;        // [n,3]
  const int* labels;       // [n]
  const int* count;        // or null
  int n;
  const float* jacobian;   // [n,A,3] or null
  float* posed;            // [M,n,3]
};

// the link bits of slot p: 1 = unused or empty (its motion is the identity), 2 = a parent it cannot hang on
__device__ __forceinline__ int pose_link_bits(const PoseArgs& a, int p, int active, int& q, int& j, double& sign) {
  int bits = 0;
  if (p >= active || (a.part_status[p] & 1)) bits |= 1;
  q = a.parent ? a.parent[p] : -1;
  j = -1;
  sign = 1.0;
  if (q >= 0) {
    j = a.joint_of[p];
    bool bad = q >= active || q == p || j < 0 || j >= counted_length(a.joints_count, a.J);
    if (!bad) {  // j < J
      const int lo = a.part_a[j], hi = a.part_b[j];
      if (lo == q && hi == p) sign = 1.0;
      else if (hi == q && lo == p) sign = -1.0;
      else bad = true;
    }
    if (bad) bits |= 2;
  }
  return bits;
}

__global__ void __launch_bounds__(NJF_POSE_THREADS) pose_links_kernel(PoseArgs a) {
  const int t = blockIdx.x * NJF_POSE_THREADS + threadIdx.x;  // M*K <= 65535 * 256 < 2^31
  if (t >= a.M * a.K) return;
  const int m = t / a.K, p = t - m * a.K;
  int q, j;
  double sign;
  const int bits = pose_link_bits(a, p, counted_length(a.parts_count, a.K), q, j, sign);
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, tr[3] = {0.0, 0.0, 0.0};
  if (bits == 0) {
    const bool hung = q >= 0;  // (then j is a stored joint)
    const double* ws = hung ? a.joint_omega + (size_t)j * a.A * 3 : a.omega + (size_t)p * a.A * 3;
    const double* vs = hung ? a.joint_velocity + (size_t)j * a.A * 3 : a.velocity + (size_t)p * a.A * 3;
    const double* cs = hung ? a.anchor + (size_t)j * 3 : a.centroid + (size_t)p * 3;
    const float* u = a.commands + (size_t)m * a.A;
    double w[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
    for (int ch = 0; ch < a.A; ++ch) {
      const double uc = (double)u[ch];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        w[c] += uc * ws[ch * 3 + c];
        v[c] += uc * vs[ch * 3 + c];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      w[c] *= sign;
      v[c] *= sign;
    }
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    double ca, cb, cg;
    if (th2 <= 1e-6) {
      const double th4 = th2 * th2;
      ca = (1.0 - th2 / 6.0) + th4 / 120.0;
      cb = (0.5 - th2 / 24.0) + th4 / 720.0;
      cg = (1.0 / 6.0 - th2 / 120.0) + th4 / 5040.0;
    } else {
      const double th = sqrt(th2), s = sin(th), sh = sin(0.5 * th);
      ca = s / th;
      cb = 2.0 * (sh * sh) / th2;       // (not 1 - cos: it cancels)
      cg = (th - s) / (th2 * th);
    }
    // [w]x and its square w w^T - th2 I
    const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    double V[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double d = r == c ? 1.0 : 0.0;
        const double W2 = w[r] * w[c] - d * th2;
        R[r * 3 + c] = (d + ca * W[r * 3 + c]) + cb * W2;
        V[r * 3 + c] = (d + cb * W[r * 3 + c]) + cg * W2;
      }
    const double c0 = cs[0], c1 = cs[1], c2 = cs[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double rc = (R[r * 3] * c0 + R[r * 3 + 1] * c1) + R[r * 3 + 2] * c2;
      const double vv = (V[r * 3] * v[0] + V[r * 3 + 1] * v[1]) + V[r * 3 + 2] * v[2];
      tr[r] = (cs[r] - rc) + vv;
    }
  }
  double* g = a.link + (size_t)t * 12;  // t < M*K
#pragma unroll
  for (int e = 0; e < 9; ++e) g[e] = R[e];
#pragma unroll
  for (int e = 0; e < 3; ++e) g[9 + e] = tr[e];
  if (m == 0) a.link_bits[p] = bits;
}

// T = G[m,p], then T <- G[m,q] o T up the parents: bounded by K steps, every index checked before it is used
__global__ void __launch_bounds__(NJF_POSE_THREADS) pose_chain_kernel(PoseArgs a) {
  const int t = blockIdx.x * NJF_POSE_THREADS + threadIdx.x;
  if (t >= a.M * a.K) return;
  const int m = t / a.K, p = t - m * a.K;
  const double* base = a.link + (size_t)m * a.K * 12;
  double T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = base[(size_t)p * 12 + e];
  const int own = a.link_bits[p];
  bool ok = !(own & 2);
  int steps = 0;
  int q = a.parent ? a.parent[p] : -1;
  while (ok && q != -1) {
    if (q < -1 || q >= a.K || steps >= a.K || (a.link_bits[q] & 2)) {  // (q checked before link_bits[q])
      ok = false;
      break;
    }
    const double* g = base + (size_t)q * 12;  // q < K
    double N[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        N[r * 3 + c] = (g[r * 3] * T[c] + g[r * 3 + 1] * T[3 + c]) + g[r * 3 + 2] * T[6 + c];
      N[9 + r] = ((g[r * 3] * T[9] + g[r * 3 + 1] * T[10]) + g[r * 3 + 2] * T[11]) + g[9 + r];
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = N[e];
    ++steps;
    q = a.parent[q];
  }
  if (!ok) {
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = (e == 0 || e == 4 || e == 8) ? 1.0 : 0.0;
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) a.rotation[(size_t)t * 9 + e] = T[e];
#pragma unroll
  for (int e = 0; e < 3; ++e) a.translation[(size_t)t * 3 + e] = T[9 + e];
  if (m == 0) {
    a.status[p] = own | (ok ? 0 : 2);
    a.depth[p] = steps;
  }
}

// One thread per row, a tile of commands per blockIdx.y.  The row's coordinates, label, slot and (for a first-order row) Jacobian
// are read once; per command the thread reads its part's 12 doubles and writes 3 floats.  STAGE: one command's transforms of
// the used slots go through LDS first (rotation and translation rows copied by the whole workgroup) instead of being read by
// every lane from L2.  WIDE: the workgroup's 3 * rows floats of a command are contiguous in the output, so they are laid out in
// LDS and written as 16-byte stores between a scalar head and tail (the output of command m starts at 12 * m * n bytes, which
// need not be a multiple of 16) instead of three dword stores per lane.
template <bool STAGE, bool WIDE>
__global__ void __launch_bounds__(NJF_POSE_THREADS) pose_points_kernel(PoseArgs a) {
  __shared__ double staged[STAGE ? NJF_FIELD_TWISTS_MAX_PARTS * 12 : 1];
  __shared__ float tile[WIDE ? NJF_POSE_THREADS * 3 : 1];
  const int rows = counted_length(a.count, a.n);
  const int tid = threadIdx.x;
  const long long first = (long long)blockIdx.x * NJF_POSE_THREADS;
  if (first >= rows) return;  // the whole workgroup, before any barrier
  const long long i = first + tid;
  const bool live = i < rows;  // (rows past the count are neither read nor written)
  const int active = counted_length(a.parts_count, a.K);
  float x = 0.f, y = 0.f, z = 0.f;
  int slot = -1;
  float jac[NJF_MAX_ACTION_DIM * 3];
#pragma unroll
  for (int e = 0; e < NJF_MAX_ACTION_DIM * 3; ++e) jac[e] = 0.f;
  if (live) {
    x = a.xyz[i * 3], y = a.xyz[i * 3 + 1], z = a.xyz[i * 3 + 2];
    const int label = a.labels[i];
    if (label >= 0) {
      const int p = cc_lower_bound(a.parts, active, label);
      if (p < active && a.parts[p] == label && a.status[p] == 0) slot = p;  // p < K
    }
    if (slot < 0 && a.jacobian) {
      const float* jr = a.jacobian + (size_t)i * a.A * 3;
#pragma unroll
      for (int ch = 0; ch < NJF_MAX_ACTION_DIM; ++ch)  // (static indices: the array stays in registers)
        if (ch < a.A) {
          jac[ch * 3] = jr[ch * 3];
          jac[ch * 3 + 1] = jr[ch * 3 + 1];
          jac[ch * 3 + 2] = jr[ch * 3 + 2];
        }
    }
  }
  const int block_rows = (int)min((long long)NJF_POSE_THREADS, rows - first);
  const int m0 = blockIdx.y * NJF_POSE_COMMAND_TILE, m1 = min(a.M, m0 + NJF_POSE_COMMAND_TILE);
  for (int m = m0; m < m1; ++m) {
    const double* rot = a.rotation + (size_t)m * a.K * 9;
    const double* trn = a.translation + (size_t)m * a.K * 3;
    if (STAGE) {
      __syncthreads();  // (the previous command's reads are done)
      for (int e = tid; e < active * 9; e += NJF_POSE_THREADS) staged[(e / 9) * 12 + e % 9] = rot[e];      // active <= K
      for (int e = tid; e < active * 3; e += NJF_POSE_THREADS) staged[(e / 3) * 12 + 9 + e % 3] = trn[e];
      __syncthreads();
    }
    float o0 = x, o1 = y, o2 = z;
    if (slot >= 0) {
      double T[12];
      if (STAGE) {
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] = staged[slot * 12 + e];
      } else {
#pragma unroll
        for (int e = 0; e < 9; ++e) T[e] = rot[(size_t)slot * 9 + e];
#pragma unroll
        for (int e = 0; e < 3; ++e) T[9 + e] = trn[(size_t)slot * 3 + e];
      }
      const double dx = (double)x, dy = (double)y, dz = (double)z;
      o0 = (float)(((T[0] * dx + T[1] * dy) + T[2] * dz) + T[9]);
      o1 = (float)(((T[3] * dx + T[4] * dy) + T[5] * dz) + T[10]);
      o2 = (float)(((T[6] * dx + T[7] * dy) + T[8] * dz) + T[11]);
    } else if (live && a.jacobian) {
      const float* u = a.commands + (size_t)m * a.A;
      double s0 = (double)x, s1 = (double)y, s2 = (double)z;
#pragma unroll
      for (int ch = 0; ch < NJF_MAX_ACTION_DIM; ++ch)
        if (ch < a.A) {
          const double uc = (double)u[ch];
          s0 += uc * (double)jac[ch * 3];
          s1 += uc * (double)jac[ch * 3 + 1];
          s2 += uc * (double)jac[ch * 3 + 2];
        }
      o0 = (float)s0, o1 = (float)s1, o2 = (float)s2;
    }
    float* out = a.posed + ((size_t)m * a.n + (size_t)first) * 3;  // the workgroup's 3 * block_rows floats of command m
    if (!WIDE) {
      if (live) {
        out[tid * 3] = o0;
        out[tid * 3 + 1] = o1;
        out[tid * 3 + 2] = o2;
      }
    } else {
      __syncthreads();  // (the previous command's tile has been written out)
      tile[tid * 3] = o0;
      tile[tid * 3 + 1] = o1;
      tile[tid * 3 + 2] = o2;
      __syncthreads();
      const int floats = block_rows * 3;
      const int head = min(floats, (int)((4 - (((size_t)out >> 2) & 3)) & 3));  // floats up to the next 16-byte boundary
      const int quads = (floats - head) >> 2;
      if (tid < head) out[tid] = tile[tid];
      if (tid < quads) {  // quads <= 192
        const int e = head + tid * 4;
        *reinterpret_cast<float4*>(out + e) = make_float4(tile[e], tile[e + 1], tile[e + 2], tile[e + 3]);
      }
      const int done = head + quads * 4;
      if (tid < floats - done) out[done + tid] = tile[done + tid];
    }
  }
}

// =============================================================================================
// inverse kinematics on the part tree: commands from 3-D point targets (njf_field_commands)
// =============================================================================================
// A part moves rigidly, so the least-squares objective sum_i w_i |R_p(u) x_i + t_p(u) - y_mi|^2, its gradient and its
// Gauss-Newton matrix depend on the rows of part p only through 23 weighted moments of (point, target).  The moments launch
// streams the rows once: workgroup (chunk, part, tile of problems) compacts the chunk's rows of the part in order (as the twists
// do), then each WAVE owns whole problems -- lane l adds list entries l, l + 64, ... and one butterfly finishes the 23 sums, so
// no barrier and no LDS traffic lies inside the loop over problems.  The finishing launch adds the chunks in ascending order
// and zeroes the parts whose pose status is not 0.  The solver launch never looks at a row: one workgroup per problem, thread p
// owns slot p.  No floating-point atomics anywhere: every sum has an order that depends on (n, K, M) alone.
#define NJF_IK_THREADS 256
#define NJF_IK_PROBLEM_TILE 16   // problems per workgroup of the moments launch (4 per wave)
#define NJF_IK_FINISH_TILE 64    // problems per workgroup of the finishing launch
#define NJF_IK_MOMENTS NJF_FIELD_COMMANDS_MOMENTS_PER_PART
// the solver's reduced entries: cost, W, g [A], H upper triangle -- at fixed places, whatever A is
#define NJF_IK_G 2
#define NJF_IK_H (NJF_IK_G + NJF_MAX_ACTION_DIM)
#define NJF_IK_ENTRIES (NJF_IK_H + NJF_MAX_ACTION_DIM * (NJF_MAX_ACTION_DIM + 1) / 2)
struct IkArgs {
  PoseArgs pose;           // the part list, twists, joints, tree and points of the pose (its outputs are unused); M = problems
  const float* targets;    // [M,n,3]
  const float* weights;    // null, [n] (weight_stride 0) or [M,n] (weight_stride n)
  long long weight_stride;
  const float* information;   // the metric entry only: [n,6] (information_stride 0) or [M,n,6] (information_stride 6 n)
  long long information_stride;
  const float *init, *lower, *upper;   // [M,A] or null
  double reg, damping;
  int iterations, chunks;
  double* partial;         // [chunks][K][M][23]
  double* link_twist;      // [M][2][K][A][6]: (W, U) per channel of every link, then of every chain, at the point being evaluated
  double* moments;         // [M][K][23]
  float* commands;         // [M,A]
  double *cost, *initial_cost, *weight, *gradient;
  int *steps, *status, *part_status, *depth;
};

// status and depth of slot p from the link bits of every slot: the walk of pose_chain_kernel without the transforms
__device__ __forceinline__ int ik_walk_status(const int* parent, const int* bits, int K, int p, int& depth) {
  const int own = bits[p];
  bool ok = !(own & 2);
  int steps = 0;
  int q = parent ? parent[p] : -1;
  while (ok && q != -1) {
    if (q < -1 || q >= K || steps >= K || (bits[q] & 2)) {  // (q checked before bits[q])
      ok = false;
      break;
    }
    ++steps;
    q = parent[q];
  }
  depth = steps;
  return own | (ok ? 0 : 2);
}

__global__ void __launch_bounds__(NJF_IK_THREADS) ik_moments_kernel(IkArgs a) {
  __shared__ int list[NJF_FIELD_TWISTS_CHUNK];
  __shared__ int wave_count[NJF_FIELD_TWISTS_CHUNK / NJF_IK_THREADS][NJF_IK_THREADS / 64];
  const PoseArgs& s = a.pose;
  const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (p >= counted_length(s.parts_count, s.K) || s.parts[p] < 0) return;  // (uniform; the finishing launch does not read it)
  const int cnt = twist_compact(s.labels, s.parts[p], counted_length(s.count, s.n), list, wave_count);
  const long long base = (long long)blockIdx.x * NJF_FIELD_TWISTS_CHUNK;
  const double c0 = s.centroid[p * 3], c1 = s.centroid[p * 3 + 1], c2 = s.centroid[p * 3 + 2];
  const int m0 = blockIdx.z * NJF_IK_PROBLEM_TILE, m1 = min(s.M, m0 + NJF_IK_PROBLEM_TILE);
  for (int m = m0 + wave; m < m1; m += NJF_IK_THREADS / 64) {
    const float* y = a.targets + (size_t)m * s.n * 3;
    const float* wt = a.weights ? a.weights + (size_t)m * a.weight_stride : nullptr;
    double* out = a.partial + (((size_t)blockIdx.x * s.K + p) * s.M + m) * NJF_IK_MOMENTS;  // p < K, m < M
    if (cnt == 0) {  // (uniform) most (chunk, slot) pairs of a cloud in grid order: the sums of nothing, without the butterflies
      if (lane < NJF_IK_MOMENTS) out[lane] = 0.0;
      continue;
    }
    double acc[NJF_IK_MOMENTS];
#pragma unroll
    for (int k = 0; k < NJF_IK_MOMENTS; ++k) acc[k] = 0.0;
    for (int e = lane; e < cnt; e += 64) {
      const long long i = base + list[e];  // a row below min(count, n)
      const float w32 = wt ? wt[i] : 1.f;
      const float y0 = y[i * 3], y1 = y[i * 3 + 1], y2 = y[i * 3 + 2];
      // (every comparison with a NaN is false: a NaN weight or target leaves the row out)
      if (w32 > 0.f && w32 < INFINITY && fabsf(y0) < INFINITY && fabsf(y1) < INFINITY && fabsf(y2) < INFINITY) {
        const double w = (double)w32;
        const double x[3] = {(double)s.xyz[i * 3] - c0, (double)s.xyz[i * 3 + 1] - c1, (double)s.xyz[i * 3 + 2] - c2};
        const double t[3] = {(double)y0 - c0, (double)y1 - c1, (double)y2 - c2};
        const double wx[3] = {w * x[0], w * x[1], w * x[2]}, wy[3] = {w * t[0], w * t[1], w * t[2]};
        acc[0] += w;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          acc[1 + c] += wx[c];
          acc[10 + c] += wy[c];
#pragma unroll
          for (int d = 0; d < 3; ++d) acc[13 + c * 3 + d] += wy[c] * x[d];
        }
        acc[4] += wx[0] * x[0];
        acc[5] += wx[0] * x[1];
        acc[6] += wx[0] * x[2];
        acc[7] += wx[1] * x[1];
        acc[8] += wx[1] * x[2];
        acc[9] += wx[2] * x[2];
        acc[22] += w * ((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
      }
    }
    double mine = 0.0;
#pragma unroll
    for (int k = 0; k < NJF_IK_MOMENTS; ++k) {
      const double v = wave_sum(acc[k]);
      if (lane == k) mine = v;
    }
    if (lane < NJF_IK_MOMENTS) out[lane] = mine;
  }
}

// ---- anisotropic targets: a 3 x 3 information per row (njf_field_commands_metric) -------------------------
// z = R x + t - y is linear in the entries of (R | t), so sum w z^T Q z, its gradient and its Gauss-Newton matrix depend on
// the rows of a part through 74 moments: s0, P[6][10] = sum (w Q_e) (x^_i x^_j), B[3][4] = sum (w b_a) x^_j, e = sum w y~.b,
// x^ = (x~, 1), b = Q y~.  The launch has ik_moments_kernel's shape; what differs is how a wave finishes its 74 sums.
#define NJF_IKM_MOMENTS NJF_FIELD_COMMANDS_METRIC_MOMENTS_PER_PART
#define NJF_IKM_P 1    // P[e][f] at 1 + 10 e + f
#define NJF_IKM_B 61   // B[a][j] at 61 + 4 a + j
#define NJF_IKM_E 73

// One step of the reduce-scatter: the L live sums of a lane are the halves lo = [0, ceil(L/2)) and hi = the rest.  A lane
// whose bit `up` is clear keeps lo and hands hi to its partner, which keeps hi and hands lo back: ceil(L/2) cross-lane moves,
// after which the lane holds the pair's sums of its half.  keep + received is own + partner's, the butterfly's v + shfl(v):
// the sum a slot ends with is the butterfly's tree over the lanes (offsets 32, 16, ..., 1), bit for bit.
template <int L>
__device__ __forceinline__ void ikm_scatter_step(double* v, int offset, bool up) {
  constexpr int lo = (L + 1) / 2;
#pragma unroll
  for (int i = 0; i < lo; ++i) {
    const double high = lo + i < L ? v[lo + i] : 0.0;  // (L odd: hi is one short; that place holds a 0 nobody stores)
    const double send = up ? v[i] : high, keep = up ? high : v[i];
    v[i] = keep + __shfl_xor(send, offset);
  }
}
// the moment that place j of a lane holds after the six steps 74 -> 37 -> 19 -> 10 -> 5 -> 3 -> 2, or -1 for a padding place
__device__ __forceinline__ int ikm_scatter_index(int lane, int j) {
  int at = j;
  bool ok = true;
  at += (lane & 1) ? 2 : 0, ok = ok && at < 3;
  at += (lane & 2) ? 3 : 0, ok = ok && at < 5;
  at += (lane & 4) ? 5 : 0, ok = ok && at < 10;
  at += (lane & 8) ? 10 : 0, ok = ok && at < 19;
  at += (lane & 16) ? 19 : 0, ok = ok && at < 37;
  at += (lane & 32) ? 37 : 0, ok = ok && at < NJF_IKM_MOMENTS;
  return ok ? at : -1;
}

template <bool BUTTERFLY>
__global__ void __launch_bounds__(NJF_IK_THREADS) ikm_moments_kernel(IkArgs a) {
  __shared__ int list[NJF_FIELD_TWISTS_CHUNK];
  __shared__ int wave_count[NJF_FIELD_TWISTS_CHUNK / NJF_IK_THREADS][NJF_IK_THREADS / 64];
  static_assert(NJF_IKM_MOMENTS == 74, "the reduce-scatter's halves are written out for 74 sums");
  const PoseArgs& s = a.pose;
  const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (p >= counted_length(s.parts_count, s.K) || s.parts[p] < 0) return;  // (uniform; the finishing launch does not read it)
  const int cnt = twist_compact(s.labels, s.parts[p], counted_length(s.count, s.n), list, wave_count);
  const long long base = (long long)blockIdx.x * NJF_FIELD_TWISTS_CHUNK;
  const double c0 = s.centroid[p * 3], c1 = s.centroid[p * 3 + 1], c2 = s.centroid[p * 3 + 2];
  const int m0 = blockIdx.z * NJF_IK_PROBLEM_TILE, m1 = min(s.M, m0 + NJF_IK_PROBLEM_TILE);
  for (int m = m0 + wave; m < m1; m += NJF_IK_THREADS / 64) {
    const float* y = a.targets + (size_t)m * s.n * 3;
    const float* wt = a.weights ? a.weights + (size_t)m * a.weight_stride : nullptr;
    const float* qs = a.information + (size_t)m * a.information_stride;
    double* out = a.partial + (((size_t)blockIdx.x * s.K + p) * s.M + m) * NJF_IKM_MOMENTS;  // p < K, m < M
    if (cnt == 0) {  // (uniform) the sums of nothing
      out[lane] = 0.0;
      if (lane + 64 < NJF_IKM_MOMENTS) out[lane + 64] = 0.0;
      continue;
    }
    double acc[NJF_IKM_MOMENTS];
#pragma unroll
    for (int k = 0; k < NJF_IKM_MOMENTS; ++k) acc[k] = 0.0;
    for (int e = lane; e < cnt; e += 64) {
      const long long i = base + list[e];  // a row below min(count, n)
      const float w32 = wt ? wt[i] : 1.f;
      const float y0 = y[i * 3], y1 = y[i * 3 + 1], y2 = y[i * 3 + 2];
      float q32[6];
      bool fine = w32 > 0.f && w32 < INFINITY && fabsf(y0) < INFINITY && fabsf(y1) < INFINITY && fabsf(y2) < INFINITY;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        q32[k] = qs[i * 6 + k];
        fine = fine && fabsf(q32[k]) < INFINITY;  // (a NaN in the information leaves the row out, like a NaN target)
      }
      if (fine) {
        const double w = (double)w32;
        const double xh[4] = {(double)s.xyz[i * 3] - c0, (double)s.xyz[i * 3 + 1] - c1, (double)s.xyz[i * 3 + 2] - c2, 1.0};
        const double t[3] = {(double)y0 - c0, (double)y1 - c1, (double)y2 - c2};
        const double q[6] = {(double)q32[0], (double)q32[1], (double)q32[2], (double)q32[3], (double)q32[4], (double)q32[5]};
        double xx[10];  // x^_i x^_j, i <= j: 00 01 02 03 11 12 13 22 23 33
        {
          int f = 0;
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = r; c < 4; ++c) xx[f++] = xh[r] * xh[c];
        }
        acc[0] += w;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const double wq = w * q[k];
#pragma unroll
          for (int f = 0; f < 10; ++f) acc[NJF_IKM_P + 10 * k + f] += wq * xx[f];
        }
        const double b[3] = {(q[0] * t[0] + q[1] * t[1]) + q[2] * t[2], (q[1] * t[0] + q[3] * t[1]) + q[4] * t[2],
                             (q[2] * t[0] + q[4] * t[1]) + q[5] * t[2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double wb = w * b[r];
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[NJF_IKM_B + 4 * r + c] += wb * xh[c];
        }
        acc[NJF_IKM_E] += w * ((t[0] * b[0] + t[1] * b[1]) + t[2] * b[2]);
      }
    }
    if (BUTTERFLY) {
      double mine[2] = {0.0, 0.0};
#pragma unroll
      for (int k = 0; k < NJF_IKM_MOMENTS; ++k) {
        const double v = wave_sum(acc[k]);
        if (lane == (k & 63)) mine[k >> 6] = v;
      }
      out[lane] = mine[0];
      if (lane + 64 < NJF_IKM_MOMENTS) out[lane + 64] = mine[1];
    } else {
      ikm_scatter_step<74>(acc, 32, lane & 32);
      ikm_scatter_step<37>(acc, 16, lane & 16);
      ikm_scatter_step<19>(acc, 8, lane & 8);
      ikm_scatter_step<10>(acc, 4, lane & 4);
      ikm_scatter_step<5>(acc, 2, lane & 2);
      ikm_scatter_step<3>(acc, 1, lane & 1);
      const int k0 = ikm_scatter_index(lane, 0), k1 = ikm_scatter_index(lane, 1);  // every k < 74 is held by one (lane, place)
      if (k0 >= 0) out[k0] = acc[0];
      if (k1 >= 0) out[k1] = acc[1];
    }
  }
}

// moments[m][p] = the chunks' partials in ascending order, or zeros for a slot whose pose status is not 0; status and depth
template <int NM>
__global__ void __launch_bounds__(NJF_IK_THREADS) ik_finish_kernel(IkArgs a) {
  __shared__ int bits[NJF_FIELD_TWISTS_MAX_PARTS];
  __shared__ int result[2];
  const PoseArgs& s = a.pose;
  const int p = blockIdx.x, tid = threadIdx.x;  // p < K
  const int active = counted_length(s.parts_count, s.K);
  for (int t = tid; t < s.K; t += NJF_IK_THREADS) {
    int q, j;
    double sign;
    bits[t] = pose_link_bits(s, t, active, q, j, sign);
  }
  __syncthreads();
  if (tid == 0) {
    int depth;
    result[0] = ik_walk_status(s.parent, bits, s.K, p, depth);
    result[1] = depth;
    if (blockIdx.y == 0) {
      a.part_status[p] = result[0];
      a.depth[p] = depth;
    }
  }
  __syncthreads();
  const bool live = result[0] == 0 && s.parts[p] >= 0;  // (status 0: p < active)
  const int m0 = blockIdx.y * NJF_IK_FINISH_TILE, items = (min(s.M, m0 + NJF_IK_FINISH_TILE) - m0) * NM;
  for (int e = tid; e < items; e += NJF_IK_THREADS) {
    const int m = m0 + e / NM, k = e % NM;  // m < M
    double sum = 0.0;
    if (live)
      for (int c = 0; c < a.chunks; ++c) sum += a.partial[(((size_t)c * s.K + p) * s.M + m) * NM + k];
    a.moments[((size_t)m * s.K + p) * NM + k] = sum;
  }
}

__device__ __forceinline__ void ik_cross(const double* x, const double* y, double* out) {
  out[0] = x[1] * y[2] - x[2] * y[1];
  out[1] = x[2] * y[0] - x[0] * y[2];
  out[2] = x[0] * y[1] - x[1] * y[0];
}
__device__ __forceinline__ double ik_dot(const double* x, const double* y) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }
__device__ __forceinline__ void ik_matvec(const double* m, const double* x, double* out) {  // m: 3 x 3 row-major
#pragma unroll
  for (int r = 0; r < 3; ++r) out[r] = (m[r * 3] * x[0] + m[r * 3 + 1] * x[1]) + m[r * 3 + 2] * x[2];
}
__device__ __forceinline__ int ik_triangle(int i, int j) {  // the place of H[i][j], i <= j, in the upper triangle
  return NJF_IK_H + i * NJF_MAX_ACTION_DIM - i * (i - 1) / 2 + (j - i);
}

__device__ __forceinline__ bool ik_entry_used(int e, int A) {  // does entry e belong to channels below A?
  if (e < NJF_IK_G) return true;
  if (e < NJF_IK_H) return e - NJF_IK_G < A;
  int i = 0, rest = e - NJF_IK_H;
  while (rest >= NJF_MAX_ACTION_DIM - i) rest -= NJF_MAX_ACTION_DIM - i, ++i;
  return i + rest < A;  // (j = i + rest >= i)
}

// One workgroup per problem, thread p owns slot p (K <= 256).  An evaluation at a point u: every thread forms its link's motion
// G (into LDS) and derivative twists (into the workspace), walks up its parents composing both, turns its part's moments into
// its share of cost, g and H, and a butterfly plus the four wave partials in wave order add the shares.  Then the A x A system
// of the robust solve's Levenberg-Marquardt rule, in double; the candidate is evaluated in full and kept if it lowers L.
// METRIC: the moments are the 74 of the anisotropic objective and the block that turns them into shares is the bilinear form
// of section 20; the links, the chain, the reduction, the rule and the Gauss-Jordan are this one text.
template <bool METRIC>
__global__ void __launch_bounds__(NJF_IK_THREADS) ik_solve_kernel(IkArgs a) {
  constexpr int NM = METRIC ? NJF_IKM_MOMENTS : NJF_IK_MOMENTS;
  __shared__ double G[NJF_FIELD_TWISTS_MAX_PARTS][12];
  __shared__ double red[NJF_IK_THREADS / 64][NJF_IK_ENTRIES];
  __shared__ double ev[NJF_IK_ENTRIES], cur[NJF_IK_ENTRIES];
  __shared__ double hmat[NJF_MAX_ACTION_DIM][NJF_MAX_ACTION_DIM + 1];
  __shared__ double grad[NJF_MAX_ACTION_DIM], lo[NJF_MAX_ACTION_DIM], hi[NJF_MAX_ACTION_DIM];
  __shared__ float u[NJF_MAX_ACTION_DIM], cand[NJF_MAX_ACTION_DIM];
  __shared__ int bits[NJF_FIELD_TWISTS_MAX_PARTS];
  __shared__ int frozen[NJF_MAX_ACTION_DIM];
  __shared__ double lam, objective, cost_now, cost_first;
  __shared__ int take, stop, accepted;
  const PoseArgs& s = a.pose;
  const int m = blockIdx.x, tid = threadIdx.x, A = s.A, K = s.K;  // m < M
  const double reg_a = a.reg / (double)A;
  const int active = counted_length(s.parts_count, K);
  int q0 = -1, j0 = -1;
  double sign = 1.0;
  if (tid < K) bits[tid] = pose_link_bits(s, tid, active, q0, j0, sign);
  if (tid < A) {
    const float l = a.lower ? a.lower[(size_t)m * A + tid] : -INFINITY, h = a.upper ? a.upper[(size_t)m * A + tid] : INFINITY;
    lo[tid] = (double)l;
    hi[tid] = (double)h;
    u[tid] = fminf(fmaxf(a.init ? a.init[(size_t)m * A + tid] : 0.f, l), h);
  }
  if (tid == 0) {
    lam = a.damping;
    accepted = 0;
  }
  __syncthreads();
  int part_state = 1, depth = 0;
  if (tid < K) {
    part_state = ik_walk_status(s.parent, bits, K, tid, depth);
    if (m == 0) {
      a.part_status[tid] = part_state;
      a.depth[tid] = depth;
    }
  }
  const bool linked = tid < K && bits[tid] == 0;  // the slot's link moves
  const bool counted = tid < K && part_state == 0 && s.parts[tid] >= 0;
  const bool hung = linked && q0 >= 0;  // (then j0 is a stored joint)
  const double* ws = hung ? s.joint_omega + (size_t)j0 * A * 3 : s.omega + (size_t)tid * A * 3;
  const double* vs = hung ? s.joint_velocity + (size_t)j0 * A * 3 : s.velocity + (size_t)tid * A * 3;
  const double* cs = hung ? s.anchor + (size_t)j0 * 3 : s.centroid + (size_t)tid * 3;
  // (W, U) of this problem's links and, after them, of its chains: [K][A][6].  A thread keeps its chain's twists here, not in
  // registers, and reads them back itself
  double* link_tw = a.link_twist + (size_t)m * 2 * K * A * 6;
  double* chain_tw = link_tw + (size_t)K * A * 6;
  const double* mom = a.moments + ((size_t)m * K + tid) * NM;  // (read by counted threads only: tid < K)

  for (int it = 0;; ++it) {
    const float* pt = it == 0 ? u : cand;
    // ---- the link: G = (R, t) as pose_links_kernel forms it, and its derivative twist (W, U) per channel --------------------
    double T[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    if (linked) {
      double w[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, 0.0};
      for (int ch = 0; ch < A; ++ch) {
        const double uc = (double)pt[ch];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          w[c] += uc * ws[ch * 3 + c];
          v[c] += uc * vs[ch * 3 + c];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        w[c] *= sign;
        v[c] *= sign;
      }
      const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
      double ca, cb, cg;
      if (th2 <= 1e-6) {
        const double th4 = th2 * th2;
        ca = (1.0 - th2 / 6.0) + th4 / 120.0;
        cb = (0.5 - th2 / 24.0) + th4 / 720.0;
        cg = (1.0 / 6.0 - th2 / 120.0) + th4 / 5040.0;
      } else {
        const double th = sqrt(th2), sn = sin(th), sh = sin(0.5 * th);
        ca = sn / th;
        cb = 2.0 * (sh * sh) / th2;
        cg = (th - sn) / (th2 * th);
      }
      double b2, g2;  // db / dth2, dg / dth2: they only steer the iteration
      if (th2 <= 1e-2) {
        b2 = (((1.0 / 907200.0) * th2 - 1.0 / 13440.0) * th2 + 1.0 / 360.0) * th2 - 1.0 / 24.0;
        g2 = (((1.0 / 9979200.0) * th2 - 1.0 / 120960.0) * th2 + 1.0 / 2520.0) * th2 - 1.0 / 120.0;
      } else {
        b2 = (ca - 2.0 * cb) / (2.0 * th2);
        g2 = (cb - 3.0 * cg) / (2.0 * th2);
      }
      const double X[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
      double V[9], D[9];  // V, and b2 [w]x + g2 [w]x^2
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double d = r == c ? 1.0 : 0.0;
          const double X2 = w[r] * w[c] - d * th2;
          T[r * 3 + c] = (d + ca * X[r * 3 + c]) + cb * X2;
          V[r * 3 + c] = (d + cb * X[r * 3 + c]) + cg * X2;
          D[r * 3 + c] = b2 * X[r * 3 + c] + g2 * X2;
        }
      double Vv[3], Dv[3], wxv[3];
      ik_matvec(V, v, Vv);
      ik_matvec(D, v, Dv);
      ik_cross(w, v, wxv);
      const double c3[3] = {cs[0], cs[1], cs[2]};
      double base[3];  // c + V v
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double rc = (T[r * 3] * c3[0] + T[r * 3 + 1] * c3[1]) + T[r * 3 + 2] * c3[2];
        T[9 + r] = (c3[r] - rc) + Vv[r];
        base[r] = c3[r] + Vv[r];
      }
      for (int ch = 0; ch < A; ++ch) {
        const double wd[3] = {sign * ws[ch * 3], sign * ws[ch * 3 + 1], sign * ws[ch * 3 + 2]};
        const double vd[3] = {sign * vs[ch * 3], sign * vs[ch * 3 + 1], sign * vs[ch * 3 + 2]};
        double W[3], Vvd[3], Wxb[3], wdxv[3], t1[3], t2[3];
        ik_matvec(V, wd, W);
        ik_matvec(V, vd, Vvd);
        ik_cross(W, base, Wxb);
        // dV v = 2 (w . w') (b2 [w]x + g2 [w]x^2) v + b w' x v + g (w' x (w x v) + w x (w' x v))
        ik_cross(wd, v, wdxv);
        ik_cross(wd, wxv, t1);
        ik_cross(w, wdxv, t2);
        const double ww = 2.0 * ik_dot(w, wd);
        const size_t at = ((size_t)tid * A + ch) * 6;  // tid < K, ch < A
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double U = (Vvd[c] - Wxb[c]) + ((ww * Dv[c] + cb * wdxv[c]) + cg * (t1[c] + t2[c]));
          link_tw[at + c] = chain_tw[at + c] = W[c];
          link_tw[at + 3 + c] = chain_tw[at + 3 + c] = U;
        }
      }
    } else if (tid < K) {  // a slot with a link bit does not move
      for (int e = 0; e < A * 6; ++e) link_tw[(size_t)tid * A * 6 + e] = chain_tw[(size_t)tid * A * 6 + e] = 0.0;
    }
    if (tid < K) {
#pragma unroll
      for (int e = 0; e < 12; ++e) G[tid][e] = T[e];
    }
    __syncthreads();  // (G and the link twists of every slot are written)
    // ---- the chain: S <- Ad_G(S) + S_q, then T <- G_q o T, up the parents ------------------------------------------------------
    if (counted) {
      int steps = 0;
      int q = s.parent ? s.parent[tid] : -1;
      while (q != -1) {
        if (q < -1 || q >= K || steps >= K) break;  // (cannot happen at status 0; every index is checked all the same)
        double g[12];  // q < K
#pragma unroll
        for (int e = 0; e < 12; ++e) g[e] = G[q][e];
        for (int ch = 0; ch < A; ++ch) {
          double* mine = chain_tw + ((size_t)tid * A + ch) * 6;
          const double* theirs = link_tw + ((size_t)q * A + ch) * 6;
          const double Wc[3] = {mine[0], mine[1], mine[2]}, Uc[3] = {mine[3], mine[4], mine[5]};
          double W[3], RU[3], Wxt[3];
          ik_matvec(g, Wc, W);
          ik_matvec(g, Uc, RU);
          ik_cross(W, g + 9, Wxt);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            mine[c] = W[c] + theirs[c];
            mine[3 + c] = (RU[c] - Wxt[c]) + theirs[3 + c];
          }
        }
        double N[12];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 3; ++c) N[r * 3 + c] = (g[r * 3] * T[c] + g[r * 3 + 1] * T[3 + c]) + g[r * 3 + 2] * T[6 + c];
          N[9 + r] = ((g[r * 3] * T[9] + g[r * 3 + 1] * T[10]) + g[r * 3 + 2] * T[11]) + g[9 + r];
        }
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] = N[e];
        ++steps;
        q = s.parent[q];
      }
    }
    // ---- the part's share of cost, W, g and H from its moments, each added over the workgroup as it is formed -------------------------
    {
      const int lane = tid & 63, wave = tid >> 6;
      auto add = [&](int e, double share) {  // (called under conditions that are the same in every thread)
        const double v = wave_sum(counted ? share : 0.0);
        if (lane == 0) red[wave][e] = v;
      };
      if constexpr (METRIC) {
        // <X, Y> = sum X_ai Y_bj P[ab][ij]; G = (R | d - c), D_k = ([W_k]x R | W_k x d + U_k), 3 x 4 each, row-major.
        // cost = <G, G> - 2 G.B + e, g_k = <D_k, G> - D_k.B, H_kl = <D_k, D_l>.  The moments are read where they are
        // used: 74 of them and ten D_k do not fit in registers next to the chain.
        const double* cp = s.centroid + (size_t)(tid < K ? tid : 0) * 3;
        const double c3[3] = {cp[0], cp[1], cp[2]};
        double d[3];
        ik_matvec(T, c3, d);
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] += T[9 + c];
        // PY = P Y: PY_ai = sum_bj P[ab][ij] Y_bj, the six blocks of P one after the other
        auto apply = [&](const double* Y, double* PY) {
#pragma unroll
          for (int e = 0; e < 12; ++e) PY[e] = 0.0;
#pragma unroll
          for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = r; c < 3; ++c) {
              const int blk = r * 3 - r * (r - 1) / 2 + (c - r);  // xx xy xz yy yz zz
              double Pe[10];
#pragma unroll
              for (int f = 0; f < 10; ++f) Pe[f] = mom[NJF_IKM_P + 10 * blk + f];
#pragma unroll
              for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                  const int lo = i < j ? i : j, hi = i < j ? j : i;
                  const double pe = Pe[lo * 4 - lo * (lo - 1) / 2 + (hi - lo)];  // 00 01 02 03 11 12 13 22 23 33
                  PY[r * 4 + i] += pe * Y[c * 4 + j];
                  if (c != r) PY[c * 4 + i] += pe * Y[r * 4 + j];
                }
            }
        };
        const double* mine = chain_tw + (size_t)(tid < K ? tid : 0) * A * 6;
        auto motion = [&](int ch, double* D) {  // D_ch, ch < A; read by counted threads only
          const double W[3] = {mine[ch * 6], mine[ch * 6 + 1], mine[ch * 6 + 2]};
          double Wxd[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {  // column c of [W]x R
            const double col[3] = {T[c], T[3 + c], T[6 + c]};
            double x[3];
            ik_cross(W, col, x);
            D[c] = x[0], D[4 + c] = x[1], D[8 + c] = x[2];
          }
          ik_cross(W, d, Wxd);
#pragma unroll
          for (int r = 0; r < 3; ++r) D[r * 4 + 3] = Wxd[r] + mine[ch * 6 + 3 + r];
        };
        double K1[12];  // P G - B
        double cost = 0.0, s0 = 0.0;
        if (counted) {
          double Gm[12], PG[12];
#pragma unroll
          for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) Gm[r * 4 + c] = T[r * 3 + c];
            Gm[r * 4 + 3] = d[r] - c3[r];
          }
          apply(Gm, PG);
          double gg = 0.0, gb = 0.0;
#pragma unroll
          for (int e = 0; e < 12; ++e) {
            const double be = mom[NJF_IKM_B + e];
            gg += Gm[e] * PG[e];
            gb += Gm[e] * be;
            K1[e] = PG[e] - be;
          }
          cost = (gg - 2.0 * gb) + mom[NJF_IKM_E];
          s0 = mom[0];
        }
        add(0, cost);
        add(1, s0);
        for (int l = 0; l < A; ++l) {
          double PD[12];
          double share = 0.0;
          if (counted) {
            double Dl[12];
            motion(l, Dl);
            apply(Dl, PD);
#pragma unroll
            for (int e = 0; e < 12; ++e) share += Dl[e] * K1[e];
          }
          add(NJF_IK_G + l, share);
          for (int k = 0; k <= l; ++k) {
            share = 0.0;
            if (counted) {
              double Dk[12];
              motion(k, Dk);
#pragma unroll
              for (int e = 0; e < 12; ++e) share += Dk[e] * PD[e];
            }
            add(ik_triangle(k, l), share);
          }
        }
      } else {
        double mo[NJF_IK_MOMENTS];
#pragma unroll
        for (int k = 0; k < NJF_IK_MOMENTS; ++k) mo[k] = counted ? mom[k] : 0.0;
        const double s0 = mo[0];
        const double* s1 = mo + 1;
        const double* t1 = mo + 10;
        const double* C = mo + 13;
        const double S2[9] = {mo[4], mo[5], mo[6], mo[5], mo[7], mo[8], mo[6], mo[8], mo[9]};
        const double* cp = s.centroid + (size_t)(tid < K ? tid : 0) * 3;
        const double c3[3] = {cp[0], cp[1], cp[2]};
        double d[3], dt[3], rs1[3], k1[3];
        ik_matvec(T, c3, d);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          d[c] += T[9 + c];
          dt[c] = d[c] - c3[c];
        }
        ik_matvec(T, s1, rs1);
        // M = R S2 R^T (symmetric), N = R C^T
        double RS[9], Mx[9], Nx[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) RS[r * 3 + c] = (T[r * 3] * S2[c] + T[r * 3 + 1] * S2[3 + c]) + T[r * 3 + 2] * S2[6 + c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            Mx[r * 3 + c] = (RS[r * 3] * T[c * 3] + RS[r * 3 + 1] * T[c * 3 + 1]) + RS[r * 3 + 2] * T[c * 3 + 2];
            Nx[r * 3 + c] = (T[r * 3] * C[c * 3] + T[r * 3 + 1] * C[c * 3 + 1]) + T[r * 3 + 2] * C[c * 3 + 2];
          }
        const double trS = (mo[4] + mo[7]) + mo[9], trM = (Mx[0] + Mx[4]) + Mx[8], trN = (Nx[0] + Nx[4]) + Nx[8];
        const double axial[3] = {Nx[5] - Nx[7], Nx[6] - Nx[2], Nx[1] - Nx[3]};  // tr([W]x N) = W . axial
        add(0, ((trS + 2.0 * ik_dot(dt, rs1)) + s0 * ik_dot(dt, dt)) - 2.0 * trN - 2.0 * ik_dot(dt, t1) + mo[22]);
        add(1, s0);
#pragma unroll
        for (int c = 0; c < 3; ++c) k1[c] = (rs1[c] + s0 * dt[c]) - t1[c];
        // beta_a = W_a x d + U_a; q_a = W_a x R s1.  tr(A_a S2 R^T) = tr([W_a]x M) is 0: M is symmetric
        const double* mine = chain_tw + (size_t)(tid < K ? tid : 0) * A * 6;
        auto twist = [&](int ch, double* W, double* beta) {  // ch < A
          double Wxd[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) W[c] = counted ? mine[ch * 6 + c] : 0.0;
          ik_cross(W, d, Wxd);
#pragma unroll
          for (int c = 0; c < 3; ++c) beta[c] = Wxd[c] + (counted ? mine[ch * 6 + 3 + c] : 0.0);
        };
        for (int i = 0; i < A; ++i) {
          double Wi[3], bi[3], qi[3], MW[3];
          twist(i, Wi, bi);
          ik_cross(Wi, rs1, qi);
          ik_matvec(Mx, Wi, MW);
          add(NJF_IK_G + i, (ik_dot(qi, dt) - ik_dot(Wi, axial)) + ik_dot(bi, k1));
          for (int j = i; j < A; ++j) {
            double Wj[3], bj[3], qj[3];
            twist(j, Wj, bj);
            ik_cross(Wj, rs1, qj);
            add(ik_triangle(i, j), ((ik_dot(Wi, Wj) * trM - ik_dot(Wj, MW)) + (ik_dot(bi, qj) + ik_dot(bj, qi))) + s0 * ik_dot(bi, bj));
          }
        }
      }
    }
    __syncthreads();
    if (tid < NJF_IK_ENTRIES)  // (the entries of channels past A were not formed: they stay 0 and are never read)
      ev[tid] = ik_entry_used(tid, A) ? ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid] : 0.0;
    __syncthreads();
    // ---- accept or reject ---------------------------------------------------------------------------------------------------------
    if (tid == 0) {
      const double W = ev[1];
      double c = W > 0.0 ? ev[0] / W : 0.0;
      c = c < 0.0 ? 0.0 : c;  // (the expansion can land a few 1e-16 E below zero; a NaN stays)
      double sq = 0.0;
      for (int k = 0; k < A; ++k) sq += (double)pt[k] * (double)pt[k];
      const double obj = c + reg_a * sq;
      if (it == 0) {
        stop = !(W > 0.0) ? NJF_FIELD_COMMANDS_NO_ROWS : (isfinite(obj) ? 0 : NJF_FIELD_COMMANDS_NOT_FINITE);
        cost_first = c;
        take = 1;
      } else {
        take = obj < objective;  // (a NaN rejects)
        accepted += take;
        lam = fmin(fmax(take ? lam / 3.0 : lam * 4.0, 1e-9), 1e9);
      }
      if (take) {
        objective = obj;
        cost_now = c;
      }
    }
    __syncthreads();
    if (take) {
      if (it > 0 && tid < A) u[tid] = cand[tid];
      if (tid < NJF_IK_ENTRIES) cur[tid] = ev[1] > 0.0 ? ev[tid] / ev[1] : 0.0;  // (cur[1] is not used)
    }
    __syncthreads();
    if (it >= a.iterations || stop) break;  // (uniform)
    // ---- the damped system: frozen coordinates, Gauss-Jordan, the clamped candidate on the fp32 lattice ------------------------------
    if (tid < A) {
      const double gi = cur[NJF_IK_G + tid] + reg_a * (double)u[tid];
      grad[tid] = gi;
      frozen[tid] = ((double)u[tid] <= lo[tid] && gi > 0.0) || ((double)u[tid] >= hi[tid] && gi < 0.0);
    }
    __syncthreads();
    const int entries = A * (A + 1);  // <= 110
    if (tid < entries) {
      const int i = tid / (A + 1), j = tid % (A + 1);
      double v;
      if (j == A)
        v = frozen[i] ? 0.0 : grad[i];
      else if (frozen[i] || frozen[j])
        v = i == j ? 1.0 : 0.0;
      else
        v = cur[ik_triangle(min(i, j), max(i, j))] + (i == j ? reg_a : 0.0);
      if (i == j) v += lam * fmax(v, 1e-12);
      hmat[i][j] = v;
    }
    __syncthreads();
    for (int p = 0; p < A; ++p) {
      double nv = 0.0;
      if (tid < entries) {
        const int i = tid / (A + 1), j = tid % (A + 1);
        const double pj = hmat[p][j] * (1.0 / hmat[p][p]);
        nv = i == p ? pj : hmat[i][j] - hmat[i][p] * pj;
      }
      __syncthreads();
      if (tid < entries) hmat[tid / (A + 1)][tid % (A + 1)] = nv;
      __syncthreads();
    }
    if (tid < A) cand[tid] = (float)fmin(fmax((double)u[tid] - hmat[tid][A], lo[tid]), hi[tid]);
    __syncthreads();
  }
  if (tid < A) {
    a.commands[(size_t)m * A + tid] = u[tid];
    a.gradient[(size_t)m * A + tid] = cur[NJF_IK_G + tid] + reg_a * (double)u[tid];
  }
  if (tid == 0) {
    a.status[m] = stop;
    a.weight[m] = ev[1];
    a.initial_cost[m] = cost_first;
    a.cost[m] = cost_now;
    a.steps[m] = accepted;
  }
}

// ---- closest points against a cell list (njf_field_nearest) -------------------------------------------
// The valid points of every observed cloud are sorted into the cells of a lattice -- counts per (problem, cell) with integer
// atomics, an exclusive scan over the Mo * C counts in three launches (sums of blocks of 1024 counts, parked in the slot of
// each block's first cell; one workgroup scans those sums; every block writes its cells' offsets and clears the counts), a
// fill that writes each point as one 16-byte record (x, y, z, j) at its cell's range -- and a query walks the Chebyshev rings
// around its own cell.  The order inside a cell depends on scheduling; the outputs do not: the arg-min of (d2, j) is the same
// in any visiting order.  Cells along z are contiguous in the list, so a column of a ring is one range of records.
#define NJF_NN_THREADS 256
#define NJF_NN_SCAN_BLOCK 1024
#define NJF_NN_SCAN_ITEMS (NJF_NN_SCAN_BLOCK / NJF_NN_THREADS)
// The list itself (DESIGN.md section 23 holds its invariants): made by cell_list_make, written by cell_list_build, read by
// the query, the moments and the voxel kernels through cell_records and cell_ring.
struct CellList {
  float origin[3];
  float cell, inv_cell;
  int dims[3];
  int C;            // cells per problem
  int Mo, T;        // clouds (1: one list for every problem), slots per cloud
  long long L;      // Mo * C < 2^31
  long long slots;  // Mo * T < 2^31
  int* start;       // [L + 1]: the first record of every (cloud, cell), the total at the end
  int* cursor;      // [L]: counts, then (zero after the scan) the fill's slot counters; free for a consumer after the build
  int4* records;    // [slots]: (x, y, z as their bits, j)
};

__device__ __forceinline__ bool nn_finite(float x, float y, float z) {
  return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;  // (NaN compares false)
}

// A posed point set and the one rule by which every entry that takes one reads a row of it (the READ ROW of include/njf_hip.h):
// below the count, finite and, with labels, of a label >= 0.
struct RowSet {
  const float* points;  // [Mq,n,3]
  const int* count;     // [1] or null
  const int* labels;    // [n] or null
  int Mq, n;
};

// row i < n of problem m: false = not read (x, y, z then hold no meaning)
__device__ __forceinline__ bool row_read(const RowSet& r, int m, long long i, float& x, float& y, float& z) {
  if (i >= counted_length(r.count, r.n)) return false;
  const float* p = r.points + ((long long)(r.Mq == 1 ? 0 : m) * r.n + i) * 3;
  x = p[0], y = p[1], z = p[2];
  if (!nn_finite(x, y, z)) return false;
  return !r.labels || r.labels[i] >= 0;
}

struct NnArgs {
  CellList list;
  RowSet rows;                // the queries
  float max_distance, max_d2;
  int* index;                 // [M,n]
  float* distance2;           // [M,n]
  int* matched;               // [M,n,3] (the bits of the floats)
  int* found;                 // [M]
};

__device__ __forceinline__ int nn_cell_axis(float p, float origin, float inv_cell, int dim) {
  const float f = floorf((p - origin) * inv_cell);
  return (int)fminf(fmaxf(f, 0.0f), (float)(dim - 1));  // dim <= 1024: exact
}

// the cell of a point: every axis clamped into the lattice
__device__ __forceinline__ void nn_cell(const CellList& l, float x, float y, float z, int& cx, int& cy, int& cz) {
  cx = nn_cell_axis(x, l.origin[0], l.inv_cell, l.dims[0]);
  cy = nn_cell_axis(y, l.origin[1], l.inv_cell, l.dims[1]);
  cz = nn_cell_axis(z, l.origin[2], l.inv_cell, l.dims[2]);
}

// FILL false: count the valid points per (problem, cell); true: write their records
template <bool FILL>
__global__ void __launch_bounds__(NJF_NN_THREADS) nn_points_kernel(CellList l, const float* observed, const int* observed_count) {
  const long long e = (long long)blockIdx.x * NJF_NN_THREADS + threadIdx.x;
  if (e >= l.slots) return;
  const int mo = (int)(e / l.T), j = (int)(e % l.T);
  if (j >= counted_length(observed_count ? observed_count + mo : nullptr, l.T)) return;
  const float* p = observed + e * 3;
  const float x = p[0], y = p[1], z = p[2];
  if (!nn_finite(x, y, z)) return;
  int cx, cy, cz;
  nn_cell(l, x, y, z, cx, cy, cz);
  const long long c = (long long)mo * l.C + ((long long)cx * l.dims[1] + cy) * l.dims[2] + cz;
  if (c < 0 || c >= l.L) return;
  if (!FILL) {
    atomicAdd(&l.cursor[c], 1);
  } else {
    const long long s = (long long)l.start[c] + atomicAdd(&l.cursor[c], 1);
    if (s >= 0 && s < l.slots) l.records[s] = make_int4(__float_as_int(x), __float_as_int(y), __float_as_int(z), j);
  }
}

// workgroup b: the sum of the counts [b * 1024, (b + 1) * 1024) to start[b * 1024]
__global__ void __launch_bounds__(NJF_NN_THREADS) nn_scan_sums_kernel(const int* counts, int* start, long long L) {
  __shared__ int wave_part[NJF_NN_THREADS / 64];
  const long long base = (long long)blockIdx.x * NJF_NN_SCAN_BLOCK + threadIdx.x * NJF_NN_SCAN_ITEMS;
  int v = 0;
#pragma unroll
  for (int e = 0; e < NJF_NN_SCAN_ITEMS; ++e)
    if (base + e < L) v += counts[base + e];
  const int s = block_sum(v, wave_part);
  if (threadIdx.x == 0) start[(long long)blockIdx.x * NJF_NN_SCAN_BLOCK] = s;
}

// workgroup b: start[c] for its 1024 cells from the block's offset and the counts, which are cleared for the fill.  A thread
// holds NJF_NN_SCAN_ITEMS consecutive cells: one item, their sum, to block_count_ranks.
__global__ void __launch_bounds__(NJF_NN_THREADS) nn_scan_cells_kernel(int* counts, int* start, long long L) {
  __shared__ int wave_part[1][NJF_NN_THREADS / 64];
  const long long base = (long long)blockIdx.x * NJF_NN_SCAN_BLOCK + threadIdx.x * NJF_NN_SCAN_ITEMS;
  int c[NJF_NN_SCAN_ITEMS], mine[1] = {0}, first[1];
#pragma unroll
  for (int e = 0; e < NJF_NN_SCAN_ITEMS; ++e) {
    c[e] = base + e < L ? counts[base + e] : 0;
    mine[0] += c[e];
  }
  // (the block's offset is read by all in front of the barrier inside, thread 0 overwrites it behind it)
  block_count_ranks(mine, start[(long long)blockIdx.x * NJF_NN_SCAN_BLOCK], first, wave_part);
  int run = first[0];
#pragma unroll
  for (int e = 0; e < NJF_NN_SCAN_ITEMS; ++e)
    if (base + e < L) {
      start[base + e] = run;
      counts[base + e] = 0;
      run += c[e];
    }
}

// The readers.  WAVE false: one lane per row (a query, or a cell); true: one wave per row, the lanes share a range's records.
// f(rec) for the records of the cells c0 .. c1 (one problem, consecutive along z): the one place that reads start and records
template <bool WAVE, class F>
__device__ __forceinline__ void cell_records(const CellList& l, long long c0, long long c1, int lane, F&& f) {
  if (c0 < 0 || c1 >= l.L || c0 > c1) return;
  long long lo = l.start[c0], hi = l.start[c1 + 1];
  lo = min(max(lo, 0LL), l.slots);
  hi = min(min(max(hi, lo), l.slots), lo + l.T);
  for (long long s = lo + (WAVE ? lane : 0); s < hi; s += WAVE ? 64 : 1) f(l.records[s]);
}

// f(rec) for the records of the Chebyshev ring r around the cell (cx, cy, cz) of the problem whose cells begin at `cells`;
// false, and nothing read: no cell at this distance, nor at a larger one
template <bool WAVE, class F>
__device__ __forceinline__ bool cell_ring(const CellList& l, long long cells, int cx, int cy, int cz, int r, int lane, F&& f) {
  const int dx = l.dims[0], dy = l.dims[1], dz = l.dims[2];
  if (cx - r < 0 && cx + r >= dx && cy - r < 0 && cy + r >= dy && cz - r < 0 && cz + r >= dz) return false;
  const int x0 = max(cx - r, 0), x1 = min(cx + r, dx - 1), y0 = max(cy - r, 0), y1 = min(cy + r, dy - 1);
  const int z0 = max(cz - r, 0), z1 = min(cz + r, dz - 1);
  for (int x = x0; x <= x1; ++x)
    for (int y = y0; y <= y1; ++y) {
      const long long column = cells + ((long long)x * dy + y) * dz;
      if (x == cx - r || x == cx + r || y == cy - r || y == cy + r) {  // a face of the ring: the whole column
        cell_records<WAVE>(l, column + z0, column + z1, lane, f);
      } else {  // (r >= 1) inside: the two ends
        if (cz - r >= 0) cell_records<WAVE>(l, column + cz - r, column + cz - r, lane, f);
        if (cz + r < dz) cell_records<WAVE>(l, column + cz + r, column + cz + r, lane, f);
      }
    }
  return true;
}

// the row of a thread (WAVE: of its wave) among the n queries of problem m, and its query
struct CellQuery {
  long long i;
  bool live;      // i < n
  bool searched;  // read by row_read
  float x, y, z;
};

template <bool WAVE>
__device__ __forceinline__ CellQuery cell_query(const RowSet& rows, int m) {
  CellQuery q{WAVE ? (long long)blockIdx.x * (NJF_NN_THREADS / 64) + (threadIdx.x >> 6)
                   : (long long)blockIdx.x * NJF_NN_THREADS + threadIdx.x,
              false, false, 0.f, 0.f, 0.f};
  q.live = q.i < rows.n;
  q.searched = q.live && row_read(rows, m, q.i, q.x, q.y, q.z);
  return q;
}

__device__ __forceinline__ long long shfl_xor_i64(long long v, int o) {  // as a pair of 32-bit halves
  const unsigned low = (unsigned)__shfl_xor((int)(unsigned)v, o, 64);
  const int high = __shfl_xor((int)(v >> 32), o, 64);
  return (long long)(((unsigned long long)(unsigned)high << 32) | low);
}

struct NnBest {
  float d2;
  int j, x, y, z;  // the record's index and the bits of its coordinates
};

#define NJF_NN_NO_INDEX 0x7fffffff  // every index j of a record or a frame point lies below it
__device__ __forceinline__ NnBest nn_none() { return NnBest{INFINITY, NJF_NN_NO_INDEX, 0, 0, 0}; }

__device__ __forceinline__ void nn_take(NnBest& b, float d2, int j, int x, int y, int z) {
  if (d2 < b.d2 || (d2 == b.d2 && j < b.j)) b = NnBest{d2, j, x, y, z};
}

// the match of one row: the best, or where it is not accepted -1, +inf and NaN
__device__ __forceinline__ void match_store(int* index, float* distance2, int* matched, long long row, bool ok, const NnBest& b) {
  const int nan = 0x7fc00000;
  index[row] = ok ? b.j : -1;
  distance2[row] = ok ? b.d2 : INFINITY;
  matched[row * 3] = ok ? b.x : nan;
  matched[row * 3 + 1] = ok ? b.y : nan;
  matched[row * 3 + 2] = ok ? b.z : nan;
}

// the lanes of the wave form agree on the best after every ring
template <bool WAVE>
__global__ void __launch_bounds__(NJF_NN_THREADS) nn_query_kernel(NnArgs a) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.y;
  const CellQuery q = cell_query<WAVE>(a.rows, m);
  const long long i = q.i;
  const bool live = q.live, searched = q.searched;
  NnBest b = nn_none();
  if (searched) {
    int cx, cy, cz;
    nn_cell(a.list, q.x, q.y, q.z, cx, cy, cz);
    const auto visit = [&](const int4 rec) {
      const float dx = q.x - __int_as_float(rec.x), dy = q.y - __int_as_float(rec.y), dz = q.z - __int_as_float(rec.z);
      nn_take(b, (dx * dx + dy * dy) + dz * dz, rec.w, rec.x, rec.y, rec.z);
    };
    // the centre cell and at most NJF_FIELD_NEAREST_MAX_RINGS rings: with ceil(max_distance / cell) + 1 <= MAX_RINGS the
    // second test below ends the search by itself, after ring MAX_RINGS at the latest
    for (int r = 0; r <= NJF_FIELD_NEAREST_MAX_RINGS; ++r) {
      if (r >= 2) {  // rings 0 .. r - 1 are done: what is left is (r - 1) cells away or more, up to rounding
        const float lim = ((float)(r - 1) - 0.0078125f) * a.list.cell;
        if (b.d2 < lim * lim || lim > a.max_distance) break;
      }
      if (!cell_ring<WAVE>(a.list, (long long)(a.list.Mo == 1 ? 0 : m) * a.list.C, cx, cy, cz, r, lane, visit)) break;
      if (WAVE)
        for (int o = 32; o > 0; o >>= 1)
          nn_take(b, __shfl_xor(b.d2, o, 64), __shfl_xor(b.j, o, 64), __shfl_xor(b.x, o, 64), __shfl_xor(b.y, o, 64),
                  __shfl_xor(b.z, o, 64));
    }
  }
  const bool writer = live && (!WAVE || lane == 0);
  const bool ok = writer && searched && b.j != NJF_NN_NO_INDEX && b.d2 <= a.max_d2;
  if (writer) match_store(a.index, a.distance2, a.matched, (long long)m * a.rows.n + i, ok, b);
  const int accepted = __popcll(__ballot(ok));
  if (lane == 0 && accepted) atomicAdd(&a.found[m], accepted);
}

// ---- surface normals from integer moments on the cell list (njf_field_normals) -----------------------------
// Every searched row reads the records of the Chebyshev rings 0 .. R around its cell -- the cell list and cell_ring's walk,
// without the best-so-far test -- and adds ten int64 sums over the points within the radius: the count, the offsets
// e = p - q quantised to k = rint(e * 2^18 / radius), and the six products k_a k_b.  The order inside a cell depends on
// scheduling; integer sums do not.  A second launch turns the sums into a covariance and takes its eigenvectors in double.
struct NrmArgs {
  CellList list;           // (the finish reads none of it)
  RowSet rows;             // the queries; labels null
  const float* viewpoint;  // [Mv,3] or null
  int Mv;
  float r2;                // (float)radius * (float)radius
  int rings;               // R
  double scale;            // 2^18 / (double)(float)radius
  int min_neighbours;
  long long* moments;      // [M,n,10]
  float* normal;           // [M,n,3]
  int* neighbours;         // [M,n]
  float* variation;        // [M,n]
  double* eigenvalues;     // [M,n,3] or null
};

// the lanes of the wave form add their sums at the end.  At most 7 waves per SIMD: the lane form fits 8 (64 VGPRs) and is then
// 4 to 8 % SLOWER from M = 16 on (section 23's measurement) -- more waves miss more often in the scattered 16-byte record loads
template <bool WAVE>
__global__ void __launch_bounds__(NJF_NN_THREADS) __attribute__((amdgpu_waves_per_eu(1, 7))) nrm_moments_kernel(NrmArgs a) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.y;
  const CellQuery q = cell_query<WAVE>(a.rows, m);
  const long long i = q.i;
  const bool live = q.live;
  long long sum[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (q.searched) {
    int cx, cy, cz;
    nn_cell(a.list, q.x, q.y, q.z, cx, cy, cz);
    // |k| <= 2^18 + 1, so k is an int and every product one 32 x 32 -> 64-bit multiply-add
    const auto visit = [&](const int4 rec) {
      const float ex = __int_as_float(rec.x) - q.x, ey = __int_as_float(rec.y) - q.y, ez = __int_as_float(rec.z) - q.z;
      if ((ex * ex + ey * ey) + ez * ez <= a.r2) {
        const int kx = (int)rint((double)ex * a.scale), ky = (int)rint((double)ey * a.scale), kz = (int)rint((double)ez * a.scale);
        sum[0] += 1;
        sum[1] += kx;
        sum[2] += ky;
        sum[3] += kz;
        sum[4] += (long long)kx * kx;
        sum[5] += (long long)kx * ky;
        sum[6] += (long long)kx * kz;
        sum[7] += (long long)ky * ky;
        sum[8] += (long long)ky * kz;
        sum[9] += (long long)kz * kz;
      }
    };
    for (int r = 0; r <= a.rings; ++r)
      if (!cell_ring<WAVE>(a.list, (long long)(a.list.Mo == 1 ? 0 : m) * a.list.C, cx, cy, cz, r, lane, visit)) break;
  }
  if (WAVE)
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
      for (int e = 0; e < 10; ++e) sum[e] += shfl_xor_i64(sum[e], o);
  if (live && (!WAVE || lane == 0)) {
    long long* out = a.moments + ((long long)m * a.rows.n + i) * 10;
#pragma unroll
    for (int e = 0; e < 10; ++e) out[e] = sum[e];
  }
}

// one Jacobi rotation on the pair (p, q) of a symmetric 3 x 3, o the third axis: zeroes a_pq; vp, vq the columns p, q of V
__device__ __forceinline__ void nrm_rotate(double& app, double& aqq, double& apq, double& aop, double& aoq, double (&vp)[3],
                                           double (&vq)[3]) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double op = aop, oq = aoq;
  aop = c * op - sn * oq;
  aoq = sn * op + c * oq;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double p = vp[k], q = vq[k];
    vp[k] = c * p - sn * q;
    vq[k] = sn * p + c * q;
  }
}

// one lane per (problem, row): the ten sums -> neighbours, normal, variation, eigenvalues.  Reads the moments only, and the
// query and the viewpoint of a row that has a normal to orient.
__global__ void __launch_bounds__(NJF_NN_THREADS) nrm_finish_kernel(NrmArgs a) {
  const int m = blockIdx.y;
  const long long i = (long long)blockIdx.x * NJF_NN_THREADS + threadIdx.x;
  if (i >= a.rows.n) return;
  const long long row = (long long)m * a.rows.n + i;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  long long N = 0;
  double lam[3] = {nan, nan, nan}, nrm[3] = {nan, nan, nan};
  bool have = false;
  if (i < counted_length(a.rows.count, a.rows.n)) {  // (rows from the count on are not read)
    const long long* s = a.moments + row * 10;
    N = s[0];
    if (N >= a.min_neighbours) {
      const double inv = (double)N;
      const double mx = (double)s[1] / inv, my = (double)s[2] / inv, mz = (double)s[3] / inv;
      // the covariance, rotated towards a diagonal; V0, V1, V2: the columns of the rotations' product, the eigenvectors
      double a00 = (double)s[4] / inv - mx * mx, a01 = (double)s[5] / inv - mx * my, a02 = (double)s[6] / inv - mx * mz;
      double a11 = (double)s[7] / inv - my * my, a12 = (double)s[8] / inv - my * mz, a22 = (double)s[9] / inv - mz * mz;
      double V0[3] = {1.0, 0.0, 0.0}, V1[3] = {0.0, 1.0, 0.0}, V2[3] = {0.0, 0.0, 1.0};
#pragma unroll 1
      for (int sweep = 0; sweep < NJF_FIELD_NORMALS_SWEEPS; ++sweep) {
        nrm_rotate(a00, a11, a01, a02, a12, V0, V1);
        nrm_rotate(a00, a22, a02, a01, a12, V0, V2);
        nrm_rotate(a11, a22, a12, a01, a02, V1, V2);
      }
      // ascending, ties in the order of the axes; the eigenvector of the smallest
      double l0 = a00, l1 = a11, l2 = a22;
      double v0 = V0[0], v1 = V0[1], v2 = V0[2];
      if (l1 < l0) {
        const double t = l0;
        l0 = l1, l1 = t;
        v0 = V1[0], v1 = V1[1], v2 = V1[2];
      }
      if (l2 < l0) {
        const double t = l0;
        l0 = l2, l2 = t;
        v0 = V2[0], v1 = V2[1], v2 = V2[2];
      }
      if (l2 < l1) {
        const double t = l1;
        l1 = l2, l2 = t;
      }
      l0 = fmax(l0, 0.0), l1 = fmax(l1, 0.0), l2 = fmax(l2, 0.0);
      const double total = (l0 + l1) + l2;
      if (total > 0.0) {
        have = true;
        const double len = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
        v0 = v0 / len, v1 = v1 / len, v2 = v2 / len;
        bool flip;
        bool seen = false;
        double toward = 0.0;
        if (a.viewpoint) {
          const float* v = a.viewpoint + (long long)(a.Mv == 1 ? 0 : m) * 3;
          const float vx = v[0], vy = v[1], vz = v[2];
          if (nn_finite(vx, vy, vz)) {
            const float* q = a.rows.points + ((long long)(a.rows.Mq == 1 ? 0 : m) * a.rows.n + i) * 3;
            seen = true;
            toward = (v0 * ((double)vx - (double)q[0]) + v1 * ((double)vy - (double)q[1])) + v2 * ((double)vz - (double)q[2]);
          }
        }
        if (seen) {
          flip = toward < 0.0;
        } else {  // the component of largest magnitude is positive, ties to the lowest axis
          double big = v0;
          if (fabs(v1) > fabs(big)) big = v1;
          if (fabs(v2) > fabs(big)) big = v2;
          flip = big < 0.0;
        }
        if (flip) v0 = -v0, v1 = -v1, v2 = -v2;
        nrm[0] = v0, nrm[1] = v1, nrm[2] = v2;
        const double s2 = a.scale * a.scale;
        lam[0] = l0 / s2, lam[1] = l1 / s2, lam[2] = l2 / s2;
        a.variation[row] = (float)(l0 / total);
      }
    }
  }
  a.neighbours[row] = (int)N;
  if (!have) a.variation[row] = (float)nan;
  a.normal[row * 3] = (float)nrm[0];
  a.normal[row * 3 + 1] = (float)nrm[1];
  a.normal[row * 3 + 2] = (float)nrm[2];
  if (a.eigenvalues) {
    a.eigenvalues[row * 3] = lam[0];
    a.eigenvalues[row * 3 + 1] = lam[1];
    a.eigenvalues[row * 3 + 2] = lam[2];
  }
}

// ---- one centroid per occupied cell (njf_field_voxels) ---------------------------------------------------------
// REDUCE reads the records of every cell of the cell list and adds, over the points whose unclamped cell is this
// cell, the fractional cell coordinates quantised to 2^-20 cells: three int64 sums and a count per cell.  The order inside a
// cell depends on scheduling; integer sums do not.  COMPACT scans the kept flags (exclusive_scan_1024) into a second starts
// array and scatters the kept cells in ascending cell index.
struct VoxArgs {
  CellList list;           // one cloud per problem; REDUCE parks the kept flags in its cursors, COMPACT's scan clears them again
  int min_points, capacity;
  long long* cell_sums;    // [L,3]
  int* cell_k;             // [L]
  const int* kept_start;   // [L + 1]: the exclusive scan of the flags
  float* points;           // [M,capacity,3]
  int* weight;             // [M,capacity]
  int* cell_index;         // [M,capacity]
  long long* sums;         // [M,capacity,3]
  int* count;              // [M]
  int* outside;            // [M]
};

// one lane, or one wave, per (problem, cell)
template <bool WAVE>
__global__ void __launch_bounds__(NJF_NN_THREADS) vox_reduce_kernel(VoxArgs a) {
  const CellList& l = a.list;
  const int lane = threadIdx.x & 63;
  const long long c = WAVE ? (long long)blockIdx.x * (NJF_NN_THREADS / 64) + (threadIdx.x >> 6)
                           : (long long)blockIdx.x * NJF_NN_THREADS + threadIdx.x;
  if (c >= l.L) return;  // (a whole wave in the wave form)
  long long sx = 0, sy = 0, sz = 0;
  int k = 0, out = 0;
  cell_records<WAVE>(l, c, c, lane, [&](const int4 rec) {
    const float tx = (__int_as_float(rec.x) - l.origin[0]) * l.inv_cell, ty = (__int_as_float(rec.y) - l.origin[1]) * l.inv_cell,
                tz = (__int_as_float(rec.z) - l.origin[2]) * l.inv_cell;
    const float fx = floorf(tx), fy = floorf(ty), fz = floorf(tz);
    const bool inside =
        fx >= 0.0f && fx < (float)l.dims[0] && fy >= 0.0f && fy < (float)l.dims[1] && fz >= 0.0f && fz < (float)l.dims[2];
    if (inside) {
      sx += (long long)rintf((tx - fx) * 1048576.0f);
      sy += (long long)rintf((ty - fy) * 1048576.0f);
      sz += (long long)rintf((tz - fz) * 1048576.0f);
    }
    k += inside, out += !inside;  // (not ++ in the two branches: through the captures that becomes a store to a selected address)
  });
  if (WAVE)
    for (int o = 32; o > 0; o >>= 1) {
      sx += shfl_xor_i64(sx, o);
      sy += shfl_xor_i64(sy, o);
      sz += shfl_xor_i64(sz, o);
      k += __shfl_xor(k, o, 64);
      out += __shfl_xor(out, o, 64);
    }
  if (!WAVE || lane == 0) {
    a.cell_sums[c * 3] = sx;
    a.cell_sums[c * 3 + 1] = sy;
    a.cell_sums[c * 3 + 2] = sz;
    a.cell_k[c] = k;
    l.cursor[c] = k >= a.min_points ? 1 : 0;
    if (out) atomicAdd(&a.outside[(int)(c / l.C)], out);
  }
}

// thread e < L: the kept cell e to its row; thread e < M * capacity: the fill of a row from the count on
__global__ void __launch_bounds__(NJF_NN_THREADS) vox_scatter_kernel(VoxArgs a) {
  const CellList& l = a.list;
  const long long e = (long long)blockIdx.x * NJF_NN_THREADS + threadIdx.x;
  if (e < l.L) {
    const int m = (int)(e / l.C), ci = (int)(e - (long long)m * l.C);
    const long long base = a.kept_start[(long long)m * l.C];
    const long long row = (long long)a.kept_start[e] - base;
    if (ci == 0) a.count[m] = (int)((long long)a.kept_start[(long long)(m + 1) * l.C] - base);
    if (a.kept_start[e + 1] > a.kept_start[e] && row >= 0 && row < a.capacity) {
      const long long r = (long long)m * a.capacity + row;
      const int k = a.cell_k[e];
      const int cz = ci % l.dims[2], cy = (ci / l.dims[2]) % l.dims[1], cx = ci / (l.dims[2] * l.dims[1]);
      const int axis[3] = {cx, cy, cz};
      const double per = (double)k * 1048576.0;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const long long s = a.cell_sums[e * 3 + d];
        a.sums[r * 3 + d] = s;
        a.points[r * 3 + d] = (float)((double)l.origin[d] + ((double)axis[d] + (double)s / per) * (double)l.cell);
      }
      a.weight[r] = k;
      a.cell_index[r] = ci;
    }
  }
  if (e < (long long)l.Mo * a.capacity) {
    const int m = (int)(e / a.capacity);
    const long long row = e - (long long)m * a.capacity;
    const long long kept = (long long)a.kept_start[(long long)(m + 1) * l.C] - a.kept_start[(long long)m * l.C];
    if (row >= kept) {
      const float nan = __int_as_float(0x7fc00000);
      a.points[e * 3] = nan, a.points[e * 3 + 1] = nan, a.points[e * 3 + 2] = nan;
      a.sums[e * 3] = 0, a.sums[e * 3 + 1] = 0, a.sums[e * 3 + 2] = 0;
      a.weight[e] = 0;
      a.cell_index[e] = -1;
    }
  }
}

// =============================================================================================
// inverse dynamics: Levenberg-Marquardt on the linearised flow, one workgroup per batch element
// =============================================================================================
// optical_flow(a) = proj(x + M a) - proj(x) with x = sum_s w x_s and M = sum_s w J_s (the composited outputs of the
// final pass; render_optical_flow, model.py:288-314).  Minimises sum_r mask_r |flow_r(a) - target_r|^2 over the command
// a -- the control loop of notebooks/real_world/2_inverse_dynamics.ipynb, which runs 100 Adam steps through
// Model.infer_optical_flow instead.  All iterations run inside ONE launch: per iteration every thread linearises its
// rays (2 x A Jacobian rows into LDS), A*A threads contract them into the normal matrix in a fixed order (no
// atomics: deterministic), thread 0 solves the damped A x A system, and the step is kept if it lowers the cost.
#define NJF_SOLVE_MAX_A 16
struct SolveArgs {
  const float* pos;     // [B,R,3]
  const float* jac;     // [B,R,3,A]
  const float* proj;    // [B,3,4]  K . inv(E)[:3]
  const float* target;  // [B,R,2]
  const float* mask;    // [B,R] or null
  const float* init;    // [B,A] or null
  int R, A, iters;
  float damping;
  float* action;        // [B,A]
};

__global__ void __launch_bounds__(256) solve_action_kernel(SolveArgs a) {
  __shared__ float rows[256][2 * NJF_SOLVE_MAX_A + 2];  // per ray: 2 Jacobian rows (A each) + 2 residuals
  __shared__ float hmat[NJF_SOLVE_MAX_A][NJF_SOLVE_MAX_A + 1];
  __shared__ float act[NJF_SOLVE_MAX_A], cand[NJF_SOLVE_MAX_A], red[256];
  __shared__ float lam, cost, cost_c;
  const int b = blockIdx.x, tid = threadIdx.x, A = a.A, R = a.R;
  const float* P = a.proj + b * 12;
  if (tid < A) act[tid] = a.init ? a.init[b * A + tid] : 0.f;
  if (tid == 0) lam = a.damping;
  __syncthreads();

  // residual (and optionally Jacobian rows) of ray r at command `cmd`; returns the squared residual
  auto eval_ray = [&](int r, const float* cmd, bool want_rows, int slot) -> float {
    const size_t ri = (size_t)b * R + r;
    const float w = a.mask ? a.mask[ri] : 1.f;
    float x[3], x0[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      x0[c] = a.pos[ri * 3 + c];
      float v = x0[c];
      for (int k = 0; k < A; ++k) v = fmaf(a.jac[(ri * 3 + c) * A + k], cmd[k], v);
      x[c] = v;
    }
    auto project = [&](const float* p, float& u, float& v, float& d) {
      const float hx = fmaf(P[2], p[2], fmaf(P[1], p[1], P[0] * p[0])) + P[3];
      const float hy = fmaf(P[6], p[2], fmaf(P[5], p[1], P[4] * p[0])) + P[7];
      d = fmaf(P[10], p[2], fmaf(P[9], p[1], P[8] * p[0])) + P[11] + 1e-9f;
      u = hx / d;
      v = hy / d;
    };
    float u0, v0, d0, u, v, d;
    project(x0, u0, v0, d0);
    project(x, u, v, d);
    const float r0 = ((u - u0) - a.target[ri * 2]) * w, r1 = ((v - v0) - a.target[ri * 2 + 1]) * w;
    if (want_rows) {
      // d uv / d x = (P[:2,:3] - uv (x) P[2,:3]) / depth, times M
      float gu[3], gv[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        gu[c] = (P[c] - u * P[8 + c]) / d;
        gv[c] = (P[4 + c] - v * P[8 + c]) / d;
      }
      for (int k = 0; k < A; ++k) {
        float ju = 0.f, jv = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float m = a.jac[(ri * 3 + c) * A + k];
          ju = fmaf(gu[c], m, ju);
          jv = fmaf(gv[c], m, jv);
        }
        rows[slot][k] = ju * w;
        rows[slot][A + k] = jv * w;
      }
      rows[slot][2 * A] = r0;
      rows[slot][2 * A + 1] = r1;
    }
    return r0 * r0 + r1 * r1;
  };
  auto block_sum = [&](float v) -> float {
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    const float out = red[0];
    __syncthreads();
    return out;
  };

  for (int it = 0; it < a.iters; ++it) {
    // normal equations H = J^T J, g = J^T res, accumulated over chunks of 256 rays in a fixed order
    // entry e = hi * (A + 1) + hj of [H | g] (hj == A: the right-hand side); A * (A + 1) <= 272 entries, so a thread
    // owns entry tid and, for A = 16, entry tid + 256 as well
    const int entries = A * (A + 1);
    float hacc[2] = {0.f, 0.f}, csum = 0.f;
    for (int r0 = 0; r0 < R; r0 += 256) {
      const int r = r0 + tid;
      if (r < R) csum += eval_ray(r, act, true, tid);
      __syncthreads();
      const int n = min(256, R - r0);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int e = tid + 256 * k;
        if (e < entries) {
          const int hi = e / (A + 1), hj = e % (A + 1);
          float acc = hacc[k];
          for (int q = 0; q < n; ++q) {
            const float bu = hj < A ? rows[q][hj] : rows[q][2 * A], bv = hj < A ? rows[q][A + hj] : rows[q][2 * A + 1];
            acc = fmaf(rows[q][hi], bu, acc);
            acc = fmaf(rows[q][A + hi], bv, acc);
          }
          hacc[k] = acc;
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = tid + 256 * k;
      if (e < entries) hmat[e / (A + 1)][e % (A + 1)] = hacc[k];
    }
    const float c_now = block_sum(csum);
    if (tid == 0) {
      cost = c_now;
      // (H + lam diag(H)) step = g, un-pivoted Gauss-Jordan (symmetric positive definite after damping)
      for (int i = 0; i < A; ++i) hmat[i][i] += lam * fmaxf(hmat[i][i], 1e-12f);
      for (int k = 0; k < A; ++k) {
        const float inv = 1.0f / hmat[k][k];
        for (int j = 0; j <= A; ++j) hmat[k][j] *= inv;
        for (int i = 0; i < A; ++i) {
          if (i == k) continue;
          const float f = hmat[i][k];
          for (int j = 0; j <= A; ++j) hmat[i][j] = fmaf(-f, hmat[k][j], hmat[i][j]);
        }
      }
      for (int i = 0; i < A; ++i) cand[i] = act[i] - hmat[i][A];
    }
    __syncthreads();
    float cs = 0.f;
    for (int r = tid; r < R; r += 256) cs += eval_ray(r, cand, false, 0);
    const float c_new = block_sum(cs);
    if (tid == 0) {
      const bool better = c_new < cost;  // NaN (a point behind the camera) compares false: step rejected
      if (better)
        for (int i = 0; i < A; ++i) act[i] = cand[i];
      lam = fminf(fmaxf(better ? lam / 3.0f : lam * 4.0f, 1e-9f), 1e9f);
    }
    __syncthreads();
  }
  if (tid < A) a.action[b * A + tid] = act[tid];
}

extern "C" int njf_solve_action(const float* mean_position, const float* jacobian, const float* projection,
                                const float* target_flow, const float* visible_mask, const float* init_action, int batch,
                                int rays, int action_dim, int iterations, float damping, float* action, void* stream) {
  if (!mean_position || !jacobian || !projection || !target_flow || !action) return NJF_E_NULL;
  if (batch < 1 || rays < 1 || iterations < 0) return NJF_E_SHAPE;
  if (action_dim < 1 || action_dim > NJF_SOLVE_MAX_A) return NJF_E_ACTION_DIM;
  SolveArgs a{mean_position, jacobian, projection, target_flow, visible_mask, init_action, rays, action_dim, iterations, damping, action};
  solve_action_kernel<<<batch, 256, 0, (hipStream_t)stream>>>(a);
  return launch_status();
}

// =============================================================================================
// robust inverse dynamics: projected IRLS Levenberg-Marquardt, one workgroup per command
// =============================================================================================
// The objective notebooks/real_world/2_inverse_dynamics.ipynb minimises with Adam, per command (group of V views):
//   L(a) = (1/N) sum_i m_i rho(r_i(a)) + (reg/A) |a|^2,  N = 2 sum_r m_r,  rho = r^2 (mse) or torch's smooth-L1,
// with a box lower <= a <= upper.  Every iteration linearises each ray as in solve_action_kernel, but scales its two
// Jacobian rows and residuals by sqrt(m omega / N), rho'(r) = omega(r) r (iteratively reweighted least squares), so the
// same fixed-order [H | g] contraction yields the IRLS normal equations; the regulariser adds (2 reg / A)(I | a).
// Coordinates on a bound whose gradient points outward are frozen (identity row and column, zero right-hand side), the
// damped system is solved by a Gauss-Jordan sweep over all A * (A + 1) entries in parallel, the candidate is clamped into
// the box, and it is kept only if the TRUE objective drops.
struct RobustSolveArgs {
  const float* pos;     // [B,R,3], B = G * V (view-major within a group)
  const float* jac;     // [B,R,3,A]
  const float* proj;    // [B,3,4]  K . inv(E)[:3] of each view
  const float* target;  // [B,R,2]
  const float* mask;    // [B,R] or null
  const float* init;    // [G,A] or null
  const float* lower;   // [G,A] or null
  const float* upper;   // [G,A] or null
  int R, A, V, iters, loss;
  float beta, reg, damping;
  float* action;        // [G,A]
};

__global__ void __launch_bounds__(256) robust_solve_kernel(RobustSolveArgs a) {
  __shared__ float rows[256][2 * NJF_SOLVE_MAX_A + 2];  // per ray: 2 weighted Jacobian rows (A each) + 2 residuals
  __shared__ float hmat[NJF_SOLVE_MAX_A][NJF_SOLVE_MAX_A + 1];
  __shared__ float act[NJF_SOLVE_MAX_A], cand[NJF_SOLVE_MAX_A], lo[NJF_SOLVE_MAX_A], hi[NJF_SOLVE_MAX_A];
  __shared__ float grad[NJF_SOLVE_MAX_A], red[256];
  __shared__ int active[NJF_SOLVE_MAX_A];
  __shared__ float lam, cost;
  const int grp = blockIdx.x, tid = threadIdx.x, A = a.A, R = a.R, VR = a.V * a.R;
  const size_t ray0 = (size_t)grp * VR;  // first ray of the group in [B,R] order
  const float reg_a = a.reg / (float)A, two_reg_a = 2.0f * reg_a;
  if (tid < A) {
    lo[tid] = a.lower ? a.lower[grp * A + tid] : -INFINITY;
    hi[tid] = a.upper ? a.upper[grp * A + tid] : INFINITY;
    act[tid] = fminf(fmaxf(a.init ? a.init[grp * A + tid] : 0.f, lo[tid]), hi[tid]);
  }
  if (tid == 0) lam = a.damping;

  auto block_sum = [&](float v) -> float {
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    const float out = red[0];
    __syncthreads();
    return out;
  };
  auto rho = [&](float e, float& omega) -> float {  // loss of one residual component and its IRLS weight
    if (a.loss == NJF_LOSS_MSE) {
      omega = 2.0f;
      return e * e;
    }
    const float ae = fabsf(e);
    if (ae < a.beta) {
      omega = 1.0f / a.beta;
      return 0.5f * e * e / a.beta;
    }
    omega = 1.0f / ae;
    return ae - 0.5f * a.beta;
  };

  float msum = 0.f;
  for (int q = tid; q < VR; q += 256) msum += a.mask ? a.mask[ray0 + q] : 1.f;
  msum = block_sum(msum);
  if (!(msum > 0.f)) {  // nothing observed: the clamped start is the answer
    if (tid < A) a.action[grp * A + tid] = act[tid];
    return;
  }
  const float inv_n = 1.0f / (2.0f * msum);

  // m * (rho(r_u) + rho(r_v)) of ray q of the group at command `cmd`, and optionally its weighted rows into LDS `slot`
  auto eval_ray = [&](int q, const float* cmd, bool want_rows, int slot) -> float {
    const size_t ri = ray0 + q;
    const float m = a.mask ? a.mask[ri] : 1.f;
    if (m == 0.f) {
      if (want_rows)
        for (int k = 0; k < 2 * A + 2; ++k) rows[slot][k] = 0.f;
      return 0.f;
    }
    const float* P = a.proj + (size_t)(grp * a.V + q / R) * 12;
    float x[3], x0[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      x0[c] = a.pos[ri * 3 + c];
      float v = x0[c];
      for (int k = 0; k < A; ++k) v = fmaf(a.jac[(ri * 3 + c) * A + k], cmd[k], v);
      x[c] = v;
    }
    auto project = [&](const float* p, float& u, float& v, float& d) {
      const float hx = fmaf(P[2], p[2], fmaf(P[1], p[1], P[0] * p[0])) + P[3];
      const float hy = fmaf(P[6], p[2], fmaf(P[5], p[1], P[4] * p[0])) + P[7];
      d = fmaf(P[10], p[2], fmaf(P[9], p[1], P[8] * p[0])) + P[11] + 1e-9f;
      u = hx / d;
      v = hy / d;
    };
    float u0, v0, d0, u, v, d;
    project(x0, u0, v0, d0);
    project(x, u, v, d);
    const float e0 = (u - u0) - a.target[ri * 2], e1 = (v - v0) - a.target[ri * 2 + 1];
    float om0, om1;
    const float l = rho(e0, om0) + rho(e1, om1);
    if (want_rows) {
      const float s0 = sqrtf(m * om0 * inv_n), s1 = sqrtf(m * om1 * inv_n);
      float gu[3], gv[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        gu[c] = (P[c] - u * P[8 + c]) / d;
        gv[c] = (P[4 + c] - v * P[8 + c]) / d;
      }
      for (int k = 0; k < A; ++k) {
        float ju = 0.f, jv = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float mk = a.jac[(ri * 3 + c) * A + k];
          ju = fmaf(gu[c], mk, ju);
          jv = fmaf(gv[c], mk, jv);
        }
        rows[slot][k] = ju * s0;
        rows[slot][A + k] = jv * s1;
      }
      rows[slot][2 * A] = e0 * s0;
      rows[slot][2 * A + 1] = e1 * s1;
    }
    return m * l;
  };

  // entry e = hi * (A + 1) + hj of [H | g]; A * (A + 1) <= 272, so a thread owns entry tid and, for A = 16, tid + 256
  const int entries = A * (A + 1);
  for (int it = 0; it < a.iters; ++it) {
    float hacc[2] = {0.f, 0.f}, csum = 0.f;
    for (int q0 = 0; q0 < VR; q0 += 256) {
      const int q = q0 + tid;
      if (q < VR) csum += eval_ray(q, act, true, tid);
      __syncthreads();
      const int n = min(256, VR - q0);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int e = tid + 256 * k;
        if (e < entries) {
          const int i = e / (A + 1), j = e % (A + 1);
          float acc = hacc[k];
          for (int q = 0; q < n; ++q) {
            const float bu = j < A ? rows[q][j] : rows[q][2 * A], bv = j < A ? rows[q][A + j] : rows[q][2 * A + 1];
            acc = fmaf(rows[q][i], bu, acc);
            acc = fmaf(rows[q][A + i], bv, acc);
          }
          hacc[k] = acc;
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = tid + 256 * k;
      if (e < entries) hmat[e / (A + 1)][e % (A + 1)] = hacc[k];
    }
    const float c_now = block_sum(csum);  // its barriers publish hmat
    // gradient with the regulariser; a coordinate on a bound whose gradient points out of the box is frozen
    if (tid < A) {
      const float gi = fmaf(two_reg_a, act[tid], hmat[tid][A]);
      grad[tid] = gi;
      active[tid] = (act[tid] <= lo[tid] && gi > 0.f) || (act[tid] >= hi[tid] && gi < 0.f);
    }
    if (tid == 0) {
      float sq = 0.f;
      for (int k = 0; k < A; ++k) sq = fmaf(act[k], act[k], sq);
      cost = fmaf(c_now, inv_n, reg_a * sq);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {  // (H + (2 reg / A) I) with frozen rows / columns, then + lam diag
      const int e = tid + 256 * k;
      if (e < entries) {
        const int i = e / (A + 1), j = e % (A + 1);
        float v = hmat[i][j];
        if (j == A)
          v = active[i] ? 0.f : grad[i];
        else if (active[i] || active[j])
          v = i == j ? 1.f : 0.f;
        else if (i == j)
          v += two_reg_a;
        if (i == j) v += lam * fmaxf(v, 1e-12f);
        hmat[i][j] = v;
      }
    }
    __syncthreads();
    // un-pivoted Gauss-Jordan (symmetric positive definite after damping), one pivot per step over all entries
    for (int p = 0; p < A; ++p) {
      float nv[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int e = tid + 256 * k;
        if (e < entries) {
          const int i = e / (A + 1), j = e % (A + 1);
          const float pj = hmat[p][j] * (1.0f / hmat[p][p]);
          nv[k] = i == p ? pj : fmaf(-hmat[i][p], pj, hmat[i][j]);
        }
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int e = tid + 256 * k;
        if (e < entries) hmat[e / (A + 1)][e % (A + 1)] = nv[k];
      }
      __syncthreads();
    }
    if (tid < A) cand[tid] = fminf(fmaxf(act[tid] - hmat[tid][A], lo[tid]), hi[tid]);
    __syncthreads();
    float cs = 0.f;
    for (int q = tid; q < VR; q += 256) cs += eval_ray(q, cand, false, 0);
    const float c_new = block_sum(cs);
    if (tid == 0) {
      float sq = 0.f;
      for (int k = 0; k < A; ++k) sq = fmaf(cand[k], cand[k], sq);
      const bool better = fmaf(c_new, inv_n, reg_a * sq) < cost;  // NaN (a point behind the camera): rejected
      if (better)
        for (int i = 0; i < A; ++i) act[i] = cand[i];
      lam = fminf(fmaxf(better ? lam / 3.0f : lam * 4.0f, 1e-9f), 1e9f);
    }
    __syncthreads();
  }
  if (tid < A) a.action[grp * A + tid] = act[tid];
}

extern "C" int njf_solve_action_robust(const float* mean_position, const float* jacobian, const float* projection,
                                       const float* target_flow, const float* visible_mask, const float* init_action,
                                       const float* lower, const float* upper, int batch, int views, int rays,
                                       int action_dim, int loss, float beta, float reg, int iterations, float damping,
                                       float* action, void* stream) {
  if (!mean_position || !jacobian || !projection || !target_flow || !action) return NJF_E_NULL;
  if (batch < 1 || rays < 1 || iterations < 0 || views < 1 || batch % views != 0) return NJF_E_SHAPE;
  if ((long long)views * rays > 0x7fffffffLL) return NJF_E_SHAPE;
  if (action_dim < 1 || action_dim > NJF_SOLVE_MAX_A) return NJF_E_ACTION_DIM;
  if (loss != NJF_LOSS_MSE && loss != NJF_LOSS_SMOOTH_L1) return NJF_E_MODE;
  if (!(beta > 0.f) || !(reg >= 0.f) || !(damping >= 0.f)) return NJF_E_VALUE;
  RobustSolveArgs a{mean_position, jacobian, projection, target_flow, visible_mask, init_action, lower, upper,
                    rays, action_dim, views, iterations, loss, beta, reg, damping, action};
  robust_solve_kernel<<<batch / views, 256, 0, (hipStream_t)stream>>>(a);
  return launch_status();
}

// =============================================================================================
// backward of the pixel-aligned bilinear sampling (training)
// =============================================================================================
// out[foot_idx[p][c]] += foot_w[p][c] * grad[p]  for the four texels of every point's footprint: the input gradient of
// F.grid_sample(bilinear, border, align_corners=True) (model_components/pixel_aligned_features.py:29-33) in hoisted
// order, i.e. on the [P, channels] latent gradient BEFORE lin_z's transpose is applied per texel.  One thread per
// (run of `run` consecutive points, channel), lane = channel: every atomic instruction of a wave covers 64 consecutive
// floats of one texel row (two full 128-byte lines; global_atomic_add_f32, no CAS loop).  Points are ordered ray-major,
// so consecutive points are neighbouring samples of one ray, which mostly fall into the same texels: each footprint
// corner keeps a running sum in a register and only issues an atomic when its texel changes (2-3x fewer atomics).
__global__ void __launch_bounds__(256) scatter_footprint_kernel(const float* __restrict__ grad, long long slice_stride,
                                                                const int* __restrict__ foot_idx,
                                                                const float* __restrict__ foot_w, int points, int run,
                                                                int channels, int row, long long total,
                                                                float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long long r = i / row;
  const int col = (int)(i - r * row);          // column of the [texels, slices * channels] output
  const int slice = col / channels, ch = col - slice * channels;
  const float* g = grad + (size_t)slice * slice_stride + ch;
  const long long p0 = r * run;
  const int n = (int)min((long long)run, (long long)points - p0);
  int cur[4] = {-1, -1, -1, -1};
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < n; ++s) {
    const size_t p = (size_t)(p0 + s);
    const float v = g[p * channels];
    const int4 idx = *(const int4*)(foot_idx + p * 4);
    const f32x4 w = *(const f32x4*)(foot_w + p * 4);
    const int t[4] = {idx.x, idx.y, idx.z, idx.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (t[c] != cur[c]) {  // wave-uniform: every lane of a wave works on the same points
        if (cur[c] >= 0) unsafeAtomicAdd(out + (size_t)cur[c] * row + col, acc[c]);
        cur[c] = t[c];
        acc[c] = 0.f;
      }
      acc[c] = fmaf(w[c], v, acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (cur[c] >= 0) unsafeAtomicAdd(out + (size_t)cur[c] * row + col, acc[c]);
}

extern "C" int njf_scatter_footprint(const float* grad, int slices, long long slice_stride, const int* foot_idx,
                                     const float* foot_w, int points, int channels, int texels, int run_length, float* out,
                                     void* stream) {
  if (!grad || !foot_idx || !foot_w || !out) return NJF_E_NULL;
  if (points < 1 || texels < 1 || channels < 1 || run_length < 1 || slices < 1 || slices > 64) return NJF_E_SHAPE;
  if ((channels & 63) && slices > 1) return NJF_E_SHAPE;  // a wave must stay inside one slice (wave-uniform footprints)
  const long long runs = ((long long)points + run_length - 1) / run_length;
  const int row = slices * channels;
  const long long total = runs * row;
  if ((total + 255) / 256 > 0x7fffffffLL) return NJF_E_SHAPE;
  scatter_footprint_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      grad, slice_stride, foot_idx, foot_w, points, run_length, channels, row, total, out);
  return launch_status();
}

// out = residual + upstream * [act > 0]  and per-block column sums of out: one layer step of the ResnetFC backward chain
// (model_components/resnet_fc.py:69-79,130-154 differentiated: the ReLU mask, the residual add and the bias gradient
// that autograd would run as compare + multiply + add + sum kernels).  A workgroup owns `rows_per_block` consecutive
// rows; a thread owns 4 consecutive channels and walks the rows in steps of 256 / (channels / 4) (8 rows per iteration
// for 128 channels): every access is a coalesced 16-byte piece of a row.
// Column sums are reduced per workgroup in a fixed order (registers -> LDS -> one row of `partial`): deterministic; the
// caller adds the few partial rows.
__global__ void __launch_bounds__(256) relu_backward_kernel(const float* __restrict__ upstream,
                                                            const float* __restrict__ act,
                                                            const float* __restrict__ residual, int points, int quads,
                                                            int rows_per_block, float* __restrict__ out,
                                                            float* __restrict__ partial) {
  __shared__ float red[256 * 4];
  const int lanes_per_row = quads;                 // threads covering one row (channels / 4)
  const int rows_per_iter = 256 / lanes_per_row;   // rows a workgroup handles per iteration
  const int tq = threadIdx.x % lanes_per_row, tr = threadIdx.x / lanes_per_row;
  const long long row0 = (long long)blockIdx.x * rows_per_block;
  const int nrows = (int)min((long long)rows_per_block, (long long)points - row0);
  f32x4 sum = {0.f, 0.f, 0.f, 0.f};
  if (tr < rows_per_iter) {
    for (int r = tr; r < nrows; r += rows_per_iter) {
      const size_t o = ((size_t)(row0 + r) * quads + tq) * 4;
      const f32x4 g = *(const f32x4*)(upstream + o);
      const f32x4 a = *(const f32x4*)(act + o);
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = a[e] > 0.f ? g[e] : 0.f;
      if (residual != nullptr) {
        const f32x4 d = *(const f32x4*)(residual + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += d[e];
      }
      *(f32x4*)(out + o) = v;
#pragma unroll
      for (int e = 0; e < 4; ++e) sum[e] += v[e];
    }
  }
  if (partial == nullptr) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) red[threadIdx.x * 4 + e] = sum[e];
  __syncthreads();
  if (threadIdx.x < lanes_per_row) {
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < rows_per_iter; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) t[e] += red[(r * lanes_per_row + threadIdx.x) * 4 + e];
    *(f32x4*)(partial + ((size_t)blockIdx.x * quads + threadIdx.x) * 4) = t;
  }
}

extern "C" int njf_relu_backward(const float* upstream, const float* act, const float* residual, int points, int channels,
                                 int rows_per_block, float* out, float* partial_colsum, void* stream) {
  if (!upstream || !act || !out) return NJF_E_NULL;
  if (points < 1 || rows_per_block < 1) return NJF_E_SHAPE;
  if (channels < 4 || (channels & 3) || channels > 1024 || (256 % (channels / 4)) != 0) return NJF_E_SHAPE;
  const long long blocks = ((long long)points + rows_per_block - 1) / rows_per_block;
  if (blocks > 0x7fffffffLL) return NJF_E_SHAPE;
  relu_backward_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(upstream, act, residual, points, channels / 4,
                                                                           rows_per_block, out, partial_colsum);
  return launch_status();
}

// ---------------------------------------------------------------------------------------------
// Epilogue of a convolution of the FROZEN encoder trunk (encoder_resnet.py:24-89: torchvision BasicBlocks in eval mode):
// out = [relu]( batch_norm_eval(x) [+ skip] ) on NCHW fp32 tensors, in ONE pass -- what the library runs as a batch-norm
// inference kernel, an add and a ReLU (2-3 launches of ~4 us each: a single-image trunk is ~115 launches whose device time is
// the launch floor, not the bytes).  batch_norm_eval(x)[c] = (x - mean[c]) / sqrt(var[c] + eps) * gamma[c] + beta[c], evaluated
// in that order (the library's).  One thread = 4 consecutive floats of one (image, channel) plane (hw % 4 == 0), or one float.
// ---------------------------------------------------------------------------------------------
struct BnActArgs {
  const float* x;
  const float *gamma, *beta, *mean, *var;
  float eps;
  const float* skip;
  int relu, channels, hw;
  long long total;   // elements
  float* out;
};

template <int V>
__global__ void __launch_bounds__(256) bn_act_kernel(BnActArgs a) {
  const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= a.total) return;
  const int c = (int)((i / a.hw) % a.channels);
  const float mean = a.mean[c], invstd = 1.0f / sqrtf(a.var[c] + a.eps), g = a.gamma[c], bta = a.beta[c];
  float v[V], sk[V];
  if constexpr (V == 4) {
    const f32x4 x4 = *(const f32x4*)(a.x + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = x4[e];
    if (a.skip) {
      const f32x4 s4 = *(const f32x4*)(a.skip + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) sk[e] = s4[e];
    }
  } else {
    v[0] = a.x[i];
    if (a.skip) sk[0] = a.skip[i];
  }
#pragma unroll
  for (int e = 0; e < V; ++e) {
    float y = (v[e] - mean) * invstd * g + bta;
    if (a.skip) y += sk[e];
    v[e] = a.relu ? fmaxf(y, 0.f) : y;
  }
  if constexpr (V == 4) {
    const f32x4 o = {v[0], v[1], v[2], v[3]};
    *(f32x4*)(a.out + i) = o;
  } else {
    a.out[i] = v[0];
  }
}

extern "C" int njf_bn_act(const float* x, const float* gamma, const float* beta, const float* running_mean,
                          const float* running_var, float eps, const float* skip, int relu, int batch, int channels, int hw,
                          float* out, void* stream) {
  if (!x || !gamma || !beta || !running_mean || !running_var || !out) return NJF_E_NULL;
  if (batch < 1 || channels < 1 || hw < 1 || !(eps >= 0.f)) return NJF_E_SHAPE;
  BnActArgs a{x, gamma, beta, running_mean, running_var, eps, skip, relu != 0, channels, hw, (long long)batch * channels * hw, out};
  hipStream_t s = (hipStream_t)stream;
  if ((hw & 3) == 0) {
    const long long threads = a.total >> 2;
    if ((threads + 255) / 256 > 0x7fffffffLL) return NJF_E_SHAPE;
    bn_act_kernel<4><<<(unsigned)((threads + 255) / 256), 256, 0, s>>>(a);
  } else {
    if ((a.total + 255) / 256 > 0x7fffffffLL) return NJF_E_SHAPE;
    bn_act_kernel<1><<<(unsigned)((a.total + 255) / 256), 256, 0, s>>>(a);
  }
  return launch_status();
}

// =============================================================================================
// backward data-gradient chain of one ResnetFC (training)
// =============================================================================================
// The reverse of resnet_tile: delta^T = W^T * upstream^T layer by layer, with the weights (transposed, packed once per
// weight update by njf_pack_resnetfc_backward) as the MFMA A operand streamed through LDS exactly like the forward pass
// and the gradient kept in the accumulator registers across all 11 layers of the net (model_components/resnet_fc.py:
// 69-79, 130-154 differentiated).  Per layer the wave reads the ReLU'd layer input the forward pass dumped (the ReLU
// mask) and writes the gradient the weight-gradient GEMM of that layer contracts with:
//   deltas[10]      = [act[10] > 0] * (W_out^T d_out)                       gradient w.r.t. h after block 4
//   deltas[2b + 1]  = [act[2b+1] > 0] * (W_fc1,b^T deltas[2b + 2])          gradient w.r.t. fc_0's output of block b
//   deltas[2b]      = deltas[2b + 2] + [act[2b] > 0] * (W_fc0,b^T deltas[2b + 1])   gradient w.r.t. h before block b
// (for b = 4 read deltas[10] where the formulas say deltas[2b + 2]).  Hence dW of the layer whose input is act[l] is
// deltas[l + 1]^T act[l] for l = 0..9, its bias gradient the column sum of deltas[l + 1], and deltas[2b] (b < 3) / deltas[0]
// are the gradients w.r.t. the hoisted latents / the lin_in output.  Exact-fp32 MFMA: gradients span many orders of
// magnitude (the split-precision forms are only exact inside fp16's range), and the work is small (0.33 MFLOP/point).
struct BackwardArgs {
  const float* d_out;   // [P, d_out_dim]
  int d_out_dim;
  const float* act;     // [11, P, 128]
  const float* w_pack;  // 21 chunks: lin_out^T | (fc_1^T, fc_0^T) of blocks 4..0
  int points;
  float* deltas;        // [11, P, 128]
  float* colsum;        // [tiles, 11, 128] per-tile column sums of deltas, or nullptr
  const unsigned* masks;  // [11, P, 4] ReLU masks the training forward dumped (then `act` is not read), or nullptr
  const float* absmax;    // device scalar max|d_out|: PREC_F16X2 (the chain runs on gradients scaled by a power of two) and deltas16
  _Float16* deltas16;     // 16-bit training storage: [11, P, 128] halves = deltas x 2^k (k from absmax as in PREC_F16X2); `deltas`
                          // is then [3, P, 128] and receives slices 0, 2, 4 only (the latent gradients the footprint scatter reads)
};

// Sum over the 32 points of a tile (lanes of one wave half) of every accumulator register, in DPP: rotate-and-add inside
// the rows of 16 lanes (afterwards every lane of a row holds the row's sum), then row_bcast:15 adds row 0 into row 1 and
// row 2 into row 3 -- lanes 16..31 / 48..63 hold the sums of the half's 64 features.  Lane 16 + 4m + q (48 + ...) then
// stores its quad: 16 predicated 16-byte stores per layer.
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_add(float v) {
  const int moved = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROWS, 0xf, true);
  return v + __builtin_bit_cast(float, moved);
}

__device__ __forceinline__ void tile_colsum(const f32x16 (&acc)[4], float* __restrict__ dst, int lane, float unscale = 1.0f) {
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = acc[m][4 * q + e];
        v = dpp_add<0x128, 0xf>(v);  // row_ror:8
        v = dpp_add<0x124, 0xf>(v);  // row_ror:4
        v = dpp_add<0x122, 0xf>(v);  // row_ror:2
        v = dpp_add<0x121, 0xf>(v);  // row_ror:1
        v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
        o[e] = v * unscale;
      }
      if ((lane & 31) == 16 + 4 * m + q) *(f32x4*)(dst + 16 * m + 4 * q) = o;
    }
}

// the same for a 64-wide tile (two accumulator blocks; dst = the layer's 64 sums + 32 * hh)
__device__ __forceinline__ void tile_colsum64(const f32x16 (&acc)[2], float* __restrict__ dst, int lane, float scale = 1.0f) {
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = acc[m][4 * q + e];
        v = dpp_add<0x128, 0xf>(v);  // row_ror:8
        v = dpp_add<0x124, 0xf>(v);  // row_ror:4
        v = dpp_add<0x122, 0xf>(v);  // row_ror:2
        v = dpp_add<0x121, 0xf>(v);  // row_ror:1
        v = dpp_add<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
        o[e] = v * scale;
      }
      if ((lane & 31) == 16 + 4 * m + q) *(f32x4*)(dst + 16 * m + 4 * q) = o;
    }
}

// acc = [act > 0] * acc (+ base), written to `dst`; act / dst address this lane's 64 features of its point.  `mask` (this lane's
// two words of the forward pass's ReLU-mask dump, dump_vec128) replaces the 16 loads of the activations by one 8-byte load: the
// chain needs the SIGN of an activation only, and reading the fp32 values back was 1.05 of the kernel's 2.81 ms on the C4 shard
template <bool ADD, bool SCALED = false>
__device__ __forceinline__ void mask_store(const float* __restrict__ act, const unsigned* __restrict__ mask, float* __restrict__ dst,
                                           bool ok, f32x16 (&acc)[4], const f32x16 (&base)[4], float unscale = 1.0f,
                                           _Float16* __restrict__ dst16 = nullptr, float scale16 = 1.0f) {
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  u32x2 bits = {0u, 0u};
  if (mask != nullptr && ok) bits = *(const u32x2*)mask;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      if (mask == nullptr && ok) a = *(const f32x4*)(act + 16 * m + 4 * q);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v;
        if (mask != nullptr) {
          // the mask bit as an all-ones / all-zeros word (v_bfe_i32: a sign-extended 1-bit field) ANDed onto the gradient's bits
          const int keep = ((int)(bits[m >> 1] << (31 - (16 * (m & 1) + 4 * q + e)))) >> 31;
          v = __int_as_float(__float_as_int(acc[m][4 * q + e]) & keep);
        } else {
          v = a[e] > 0.f ? acc[m][4 * q + e] : 0.f;
        }
        if (ADD) v += base[m][4 * q + e];
        acc[m][4 * q + e] = v;
        o[e] = SCALED ? v * unscale : v;   // (a power of two: exact)
      }
      if (ok && dst != nullptr) *(f32x4*)(dst + 16 * m + 4 * q) = o;
    }
  if (dst16 != nullptr && ok) {   // (wave-uniform) the same values x 2^k as fp16: 8 stores of 16 bytes
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          o[e] = pack_pair_f16<false>(acc[m][8 * q + 2 * e] * scale16, acc[m][8 * q + 2 * e + 1] * scale16);
        *(u32x4*)(dst16 + 16 * m + 8 * q) = o;
      }
  }
}

template <int PREC>
__global__ void __launch_bounds__(NJF_THREADS, 2) resnetfc_backward_kernel(BackwardArgs a) {
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, j = lane & 31, hh = lane >> 5;
  const int tile = blockIdx.x * NJF_WAVES + wave;
  const int p = tile * 32 + j;
  const bool ok = p < a.points;
  const size_t pc = (size_t)min(p, a.points - 1);
  const size_t layer = (size_t)a.points * 128;
  const float* act = a.act ? a.act + pc * 128 + 64 * hh : nullptr;
  const unsigned* msk = a.masks ? a.masks + pc * 4 + 2 * hh : nullptr;
  const size_t mlayer = (size_t)a.points * 4;
  float* out = a.deltas + pc * 128 + 64 * hh;
  float* sums = a.colsum ? a.colsum + (size_t)tile * (11 * 128) + 64 * hh : nullptr;
  WeightStream st;
  stream_begin(st, a.w_pack, 21, 1, wave, lane);
  // PREC_F16X2 (opt-in; training.py: backward_precision): every product is hi*hi + hi*lo + lo*hi of fp16 halves, fp32-class (2^-22)
  // only inside fp16's range -- gradients are 1e-3 ... 1e-9.  The chain is LINEAR in d_out, so it runs on d_out * 2^k with k chosen
  // from max|d_out| (device scalar `absmax`, one reduction in front of the launch) such that the largest entry becomes 64: 2^9 of
  // head room before fp16's 65504, full 22 bits for entries down to 2^-9 of the largest and >= 11 bits down to 2^-20 of it (what
  // the smaller ones contribute to a weight gradient is below that in absolute terms); results are scaled back on the way out
  // (powers of two: exact).  The reference itself trains on TF32 products (train.py:64-65: 10 mantissa bits).
  constexpr bool SCALED = PREC != PREC_F32;
  float scale = 1.0f, unscale = 1.0f;   // of the chain's own arithmetic
  float pow2 = 1.0f;                    // 2^k of max|d_out| (what the fp16 deltas are scaled by, in either product form)
  if (SCALED || a.deltas16 != nullptr) {
    const float mx = a.absmax ? *a.absmax : 0.f;
    if (mx > 0.f && mx < 3.0e38f) {
      int e;
      frexpf(mx, &e);                      // mx = f * 2^e, f in [0.5, 1)
      const int k = max(min(6 - e, 120), -120);
      pow2 = ldexpf(1.0f, k);
      if (SCALED) {
        scale = pow2;
        unscale = ldexpf(1.0f, -k);
      }
    }
  }
  const float scale16 = SCALED ? 1.0f : pow2;   // the accumulators already carry 2^k in the split-precision form
  _Float16* out16 = a.deltas16 ? a.deltas16 + pc * 128 + 64 * hh : nullptr;
  const bool compact = a.deltas16 != nullptr;   // fp32 deltas: slices 0, 2, 4 only, stored as [3, P, 128]
  f32x16 din[1];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int d = 16 * hh + r;
    din[0][r] = (ok && d < a.d_out_dim) ? a.d_out[pc * a.d_out_dim + d] * scale : 0.f;
  }
  f32x16 delta[4], t[4], u[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) delta[m] = (f32x16)(0.f);
  {
    const float* wl = stream_step(st, wave, lane);
    mma_chunk<PREC, 4, 1, 0, false, 1>(st, wl, lane, din, delta);   // lin_out^T (first half of the chunk)
  }
  mask_store<false, SCALED>(act + 10 * layer, msk ? msk + 10 * mlayer : nullptr, compact ? nullptr : out + 10 * layer, ok, delta, delta,
                            unscale, out16 ? out16 + 10 * layer : nullptr, scale16);
  const bool live = tile * 32 < a.points;  // wave-uniform
  if (sums && live) tile_colsum(delta, sums + 10 * 128, lane, unscale);
  for (int blk = 4; blk >= 0; --blk) {
#pragma unroll
    for (int m = 0; m < 4; ++m) t[m] = (f32x16)(0.f);
    {
      const float* wl = stream_step(st, wave, lane);
      mma_chunk<PREC, 4, 2, 0, false, 4>(st, wl, lane, delta, t);
    }
    {
      const float* wl = stream_step(st, wave, lane);
      mma_chunk<PREC, 4, 2, 2, false, 4>(st, wl, lane, delta, t);
    }
    mask_store<false, SCALED>(act + (size_t)(2 * blk + 1) * layer, msk ? msk + (size_t)(2 * blk + 1) * mlayer : nullptr,
                              compact ? nullptr : out + (size_t)(2 * blk + 1) * layer, ok, t, t, unscale,
                              out16 ? out16 + (size_t)(2 * blk + 1) * layer : nullptr, scale16);
    if (sums && live) tile_colsum(t, sums + (2 * blk + 1) * 128, lane, unscale);
#pragma unroll
    for (int m = 0; m < 4; ++m) u[m] = (f32x16)(0.f);
    {
      const float* wl = stream_step(st, wave, lane);
      mma_chunk<PREC, 4, 2, 0, false, 4>(st, wl, lane, t, u);
    }
    {
      const float* wl = stream_step(st, wave, lane);
      mma_chunk<PREC, 4, 2, 2, false, 4>(st, wl, lane, t, u);
    }
    mask_store<true, SCALED>(act + (size_t)(2 * blk) * layer, msk ? msk + (size_t)(2 * blk) * mlayer : nullptr,
                             compact ? (blk < 3 ? out + (size_t)blk * layer : nullptr) : out + (size_t)(2 * blk) * layer, ok, u, delta,
                             unscale, out16 ? out16 + (size_t)(2 * blk) * layer : nullptr, scale16);
    if (sums && live) tile_colsum(u, sums + (2 * blk) * 128, lane, unscale);
#pragma unroll
    for (int m = 0; m < 4; ++m) delta[m] = u[m];
  }
}

extern "C" int njf_pack_resnetfc_backward(const NjfResnetFcWeights* src, float* w_out, int precision, void* stream) {
  if (!src || !w_out) return NJF_E_NULL;
  if (precision != NJF_PRECISION_F32 && precision != NJF_PRECISION_F16X2) return NJF_E_MODE;
  if (src->d_out < 1 || src->d_out > 32) return NJF_E_DOUT;
  if (!src->lin_out_w) return NJF_E_NULL;
  for (int i = 0; i < 5; ++i)
    if (!src->fc0_w[i] || !src->fc1_w[i]) return NJF_E_NULL;
  hipStream_t s = (hipStream_t)stream;
  const int P = precision;
  PackScope scope(s);   // 11 transposed layers: one launch
  // chunk 0: lin_out^T  [128 x d_out -> 32], half a chunk; the other half is never read but is moved by the DMA
  launch_pack(src->lin_out_w, nullptr, 128, src->d_out, 4, 1, 3, P, w_out, nullptr, s);
  fill_kernel<<<16, 256, 0, s>>>(w_out + 4096, 4096, 0.f);
  for (int blk = 4, c = 1; blk >= 0; --blk, c += 4) {
    launch_pack(src->fc1_w[blk], nullptr, 128, 128, 4, 4, 3, P, w_out + (size_t)c * NJF_CHUNK_FLOATS, nullptr, s);
    launch_pack(src->fc0_w[blk], nullptr, 128, 128, 4, 4, 3, P, w_out + (size_t)(c + 2) * NJF_CHUNK_FLOATS, nullptr, s);
  }
  scope.flush();   // (before the status query: a failed batch launch must be this call's error)
  return launch_status();
}

// =============================================================================================
// Backward of the folded Jacobian transformer head (transformer_tile): the data-gradient chain of its three layers in ONE launch,
// in exact fp32 MFMA.  Per layer l (x = residual stream in front of it, dumped by the training forward; dx = gradient behind it):
//   forward again:  n = norm(x);  a = softmax_8(Mqk n + bqk);  xm = x + Nov a + bo;  n2 = norm(xm);  u = W1' n2 + b1';  h = gelu(u)
//   backward:       du  = (W2^T dx) * gelu'(u)                      dxm = dx + norm'(W1'^T du ; n2)
//                   ds  = softmax'(a ; Nov^T dxm)                   dx  = dxm + norm'(Mqk^T ds ; n)     (= gradient in front of l)
// and, like njf_resnetfc_backward, it EMITS per layer the pairs a weight gradient contracts over the points (K = points: one
// batched library GEMM on the host): X = (n, a, n2, h) and dY = (ds, dxm, du, dx) for (Mqk, Nov, W1', W2).  What autograd runs for
// the reference's parameterisation of the same head (transformer.py:38-135 recomputed in library ops: 54 ms of a 62 ms action
// step on SURVEY's C4 shard) -- the gradients of the FOLDED matrices go back to the reference's parameters through the fold's
// own autograd graph on the host (64 x 64 matrices).
// Weight blob (13 chunks, two 64 x 64 matrices each): [Wj^T | -] then for l = 2, 1, 0: [Mqk | Nov] [W1' | W2^T] [W1'^T | Nov^T]
// [Mqk^T | -];  bias blob [3][192] = (bqk | bo | b1') per layer.
// =============================================================================================

struct TransformerBwdArgs {
  const float* x;        // [4, P, 64] residual stream (NjfRenderOutputs.jac_act of a transformer-head training forward)
  const float* d_out;    // [P, d_out_dim]
  int d_out_dim, keys, points;
  const float* w_pack;   // NJF_TRANSFORMER_BACKWARD_CHUNKS chunks
  const float* b_pack;   // [3][192]
  float* wg_x;           // [12, P, 64]  X of (Mqk, Nov, W1', W2) of layer l at 4l + (0, 1, 2, 3)
  float* wg_dy;          // [12, P, 64]  dY, same order
  float* dx0;            // [P, 64] gradient w.r.t. the head's input (query MLP output)
  float* colsum;         // [tiles, 12, 64] per-tile column sums of the dY (the bias gradients), or nullptr
  // 16-bit training storage (training.py: what the weight-gradient GEMMs read): wg_x / wg_dy address HALVES, the dY are stored
  // x 2^k with k = 6 - exponent(max|d_out|) as in njf_resnetfc_backward (the caller divides the GEMM's result by 2^k)
  int half;
  const float* absmax;   // device scalar max|d_out| (half storage only)
};

// this lane's 32 values as halves (x scale): 4 stores of 16 bytes at row + 32 * hh (in halves)
__device__ __forceinline__ void store_vec64_f16(_Float16* __restrict__ dst, const f32x16 (&v)[2], float scale) {
  if (dst == nullptr) return;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = pack_pair_f16<false>(v[m][8 * q + 2 * e] * scale, v[m][8 * q + 2 * e + 1] * scale);
      *(u32x4*)(dst + 16 * m + 8 * q) = o;
    }
}

// PREC_F16X2 (opt-in like resnetfc_backward_kernel<PREC_F16X2>; training.py: backward_precision): every product -- the layer's
// re-evaluation and the chain -- is hi*hi + hi*lo + lo*hi of fp16 halves.  The re-evaluated activations are O(1) (the forward pass
// runs the same products in the same form); the chain is linear in d_out and runs on d_out * 2^k, k = 6 - exponent(max|d_out|), the
// dY / dx0 / column sums are scaled back on the way out (fp16 pairs keep the 2^k, as in the exact form).
template <int PREC>
__global__ void __launch_bounds__(NJF_THREADS, 2) transformer_backward_kernel(TransformerBwdArgs a) {
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, j = lane & 31, hh = lane >> 5;
  const int tile = blockIdx.x * NJF_WAVES + wave;
  const int p = tile * 32 + j;
  const bool ok = p < a.points;
  const size_t pc = (size_t)min(p, a.points - 1);
  const size_t slice = (size_t)a.points * 64;
  const size_t row = pc * 64 + 32 * hh;
  load_bias_block(a.b_pack, 3 * 192, 0);
  WeightStream st;
  stream_begin(st, a.w_pack, NJF_TRANSFORMER_BACKWARD_CHUNKS, 1, wave, lane);
  const float* bias = njf_lds + LDS_BIAS;
  float* const wx = !ok ? nullptr : (a.half ? (float*)((_Float16*)a.wg_x + row) : a.wg_x + row);
  float* const wy = !ok ? nullptr : (a.half ? (float*)((_Float16*)a.wg_dy + row) : a.wg_dy + row);
  constexpr bool SCALED = PREC != PREC_F32;
  float pow2 = 1.0f, unpow2 = 1.0f;   // 2^k of max|d_out| and its inverse (wave-uniform)
  if (SCALED || a.half) {
    const float mx = a.absmax ? *a.absmax : 0.f;
    if (mx > 0.f && mx < 3.0e38f) {
      int e;
      frexpf(mx, &e);
      const int k = max(min(6 - e, 120), -120);
      pow2 = ldexpf(1.0f, k);
      unpow2 = ldexpf(1.0f, -k);
    }
  }
  const bool half = a.half != 0;
  const float scale = SCALED ? pow2 : 1.0f;                                     // of the chain's own arithmetic
  const float unscale = SCALED ? unpow2 : 1.0f;                                 // what leaves the chain in fp32
  const float dy_scale = half ? (SCALED ? 1.0f : pow2) : unscale;               // of a stored dY
  // the (X, dY) pair slots: fp32, or halves under the 16-bit training storage (X as it is, dY x 2^k)
  auto put = [&](float* base, int k, const f32x16 (&v)[2], float scale) {
    if (base == nullptr) return;
    if (half) store_vec64_f16((_Float16*)base + (size_t)k * slice, v, scale);
    else if (SCALED && scale != 1.0f) {
      f32x16 w[2] = {v[0] * scale, v[1] * scale};
      store_vec64(base + (size_t)k * slice, w);
    } else store_vec64(base + (size_t)k * slice, v);
  };
  // (rows of padding lanes contribute nothing: their d_out is zero and the chain is linear in it)
  float* const sums = (a.colsum && tile * 32 < a.points) ? a.colsum + (size_t)tile * (12 * 64) + 32 * hh : nullptr;

  f32x16 din[1];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int d = 16 * hh + r;
    din[0][r] = (ok && d < a.d_out_dim) ? a.d_out[pc * a.d_out_dim + d] * scale : 0.f;
  }
  f32x16 dx[2], xin[2], n[2], t[2], n2[2], u[2];
  dx[0] = (f32x16)(0.f);
  dx[1] = (f32x16)(0.f);
  const float* wl = stream_step(st, wave, lane);
  mma_chunk<PREC, 2, 1, 0, false, 1>(st, wl, lane, din, dx);   // Wj^T: gradient behind layer 2
  for (int l = 2; l >= 0; --l) {
    const float* bl = bias + 192 * l;
    load_vec64(a.x + (size_t)l * slice + row, true, xin);
    // ---- the layer again -----------------------------------------------------------------------------------------
    const float rstd1 = norm64_rstd(xin, n);
    put(wx, 4 * l + 0, n, 1.0f);
    bias_init<2, true, PREC>(bl, hh, t);
    wl = stream_step(st, wave, lane);
    mma_chunk<PREC, 2, 2, 0, false, 2>(st, wl, lane, n, t);            // dots[head * 8 + key]
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int h8 = 0; h8 < 2; ++h8) {
        float mx = -3.0e38f;
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k < a.keys) mx = fmaxf(mx, t[m][8 * h8 + k]);
        float e[8], sum = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          e[k] = (k < a.keys) ? __builtin_amdgcn_exp2f((t[m][8 * h8 + k] - mx) * 1.4426950408889634f) : 0.f;
          sum += e[k];
        }
        const float inv = 1.0f / sum;
#pragma unroll
        for (int k = 0; k < 8; ++k) t[m][8 * h8 + k] = e[k] * inv;       // a
      }
    put(wx, 4 * l + 1, t, 1.0f);
    // Nov a + bo on an accumulator of its own (u is free here), added to x once: 64 small terms accumulated onto the residual
    // stream itself are 64 roundings at ulp(x), several times what one fp32 addition of the finished product costs
    bias_init<2, true, PREC>(bl + 64, hh, u);
    mma_chunk<PREC, 2, 2, 0, false, 2>(st, wl + 4096, lane, t, u);
    xin[0] += u[0];
    xin[1] += u[1];                                                          // xm = x + (Nov a + bo)
    const float rstd2 = norm64_rstd(xin, n2);
    put(wx, 4 * l + 2, n2, 1.0f);
    u[0] = (f32x16)(0.f);
    u[1] = (f32x16)(0.f);
    wl = stream_step(st, wave, lane);
    mma_chunk<PREC, 2, 2, 0, false, 2>(st, wl, lane, n2, u);
    bias_init<2, false, PREC>(bl + 128, hh, u);                              // u = (W1' n2) + b1': the bias, too, is added once
    {
      f32x16 hval[2];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = u[m][r];
          const float cdf = 0.5f * (1.0f + erf_branchless(v * 0.70710678118654752440f));
          hval[m][r] = v * cdf;                                             // gelu(u)
          // gelu'(u) = Phi(u) + u phi(u),  phi(u) = exp(-u^2 / 2) / sqrt(2 pi)
          u[m][r] = fmaf(v * 0.3989422804014327f, __builtin_amdgcn_exp2f(v * v * -0.7213475204444817f), cdf);
        }
      put(wx, 4 * l + 3, hval, 1.0f);
    }
    // ---- and backwards ---------------------------------------------------------------------------------------------
    put(wy, 4 * l + 3, dx, dy_scale);                                    // W2:  dY = dx
    if (sums) tile_colsum64(dx, sums + (4 * l + 3) * 64, lane, unscale);
    xin[0] = (f32x16)(0.f);
    xin[1] = (f32x16)(0.f);
    mma_chunk<PREC, 2, 2, 0, false, 2>(st, wl + 4096, lane, dx, xin);   // W2^T dx
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) u[m][r] *= xin[m][r];                     // du
    put(wy, 4 * l + 2, u, dy_scale);                                     // W1': dY = du
    if (sums) tile_colsum64(u, sums + (4 * l + 2) * 64, lane, unscale);
    xin[0] = (f32x16)(0.f);
    xin[1] = (f32x16)(0.f);
    wl = stream_step(st, wave, lane);
    mma_chunk<PREC, 2, 2, 0, false, 2>(st, wl, lane, u, xin);           // W1'^T du = dn2
    norm64_backward(xin, n2, rstd2, dx);                                     // dxm = dx + norm'(dn2)
    put(wy, 4 * l + 1, dx, dy_scale);                                    // Nov: dY = dxm
    if (sums) tile_colsum64(dx, sums + (4 * l + 1) * 64, lane, unscale);
    xin[0] = (f32x16)(0.f);
    xin[1] = (f32x16)(0.f);
    mma_chunk<PREC, 2, 2, 0, false, 2>(st, wl + 4096, lane, dx, xin);   // Nov^T dxm = da
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int h8 = 0; h8 < 2; ++h8) {
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) dot = fmaf(t[m][8 * h8 + k], xin[m][8 * h8 + k], dot);
#pragma unroll
        for (int k = 0; k < 8; ++k) t[m][8 * h8 + k] *= xin[m][8 * h8 + k] - dot;   // ds = a (da - <a, da>)
      }
    put(wy, 4 * l + 0, t, dy_scale);                                     // Mqk: dY = ds
    if (sums) tile_colsum64(t, sums + (4 * l + 0) * 64, lane, unscale);
    xin[0] = (f32x16)(0.f);
    xin[1] = (f32x16)(0.f);
    wl = stream_step(st, wave, lane);
    mma_chunk<PREC, 2, 2, 0, false, 2>(st, wl, lane, t, xin);           // Mqk^T ds = dn
    norm64_backward(xin, n, rstd1, dx);                                      // gradient in front of layer l
  }
  if (ok) {
    if (SCALED) {
      dx[0] *= unscale;
      dx[1] *= unscale;
    }
    store_vec64(a.dx0 + row, dx);
  }
}

// =============================================================================================
// stand-alone sampler ops
// =============================================================================================
__global__ void __launch_bounds__(256) alpha_weights_kernel(const float* __restrict__ deltas,
                                                            const float* __restrict__ dens, int rays, int samples,
                                                            float* __restrict__ weights) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // one wave per ray, both halves duplicate
  const int lane = threadIdx.x & 63, j = lane & 31;
  if (wave >= rays) return;
  float carry = 0.f;
  for (int t = 0; t * 32 < samples; ++t) {
    const int s = t * 32 + j;
    const bool valid = s < samples;
    const size_t i = (size_t)wave * samples + min(s, samples - 1);
    const float w = tile_weights(deltas[i], dens[i], valid, j, carry);
    if (valid && lane < 32) weights[i] = w;
  }
}

extern "C" int njf_alpha_weights(const float* deltas, const float* densities, int rays, int samples, float* weights,
                                 void* stream) {
  if (!deltas || !densities || !weights) return NJF_E_NULL;
  if (rays < 1 || samples < 1) return NJF_E_SHAPE;
  alpha_weights_kernel<<<(rays + 3) / 4, 256, 0, (hipStream_t)stream>>>(deltas, densities, rays, samples, weights);
  return launch_status();
}

// ---------------------------------------------------------------------------------------------
// Backward of alpha compositing (training, perception mode): what autograd runs for RaySamples.get_weights
// (ray_samplers.py:77-101) + render_rgb + the un-clipped render_depth (model.py:257-279) -- where / mul / cumsum / cat /
// exp / exp / sub / mul / sum ... ~25 launches per level -- as ONE launch.  With ds_s = delta_s sigma_s (0 where delta <= 0),
// T_s = exp(-sum_{j<s} ds_j), w_s = (1 - exp(-ds_s)) T_s:
//   G_s        = g_w[s] + g_rgb . c_s + g_depth (t_s - depth) / (sum w + 1e-10)      (total derivative w.r.t. w_s)
//   dL/dds_k   = G_k T_{k+1} - sum_{s>k} G_s w_s                                      (dw_s/dds_s = T_{s+1}, dw_s/dds_k = -w_s)
//   dL/dsigma_k = delta_k dL/dds_k,   dL/dc_k = w_k g_rgb
// One wave per ray, lane = sample inside a tile of 64; a forward sweep over the tiles (prefix sums -> T, w, sum w, sum w t)
// and a reverse sweep (suffix sums of G w), both with fixed orders: bit-reproducible.
// ---------------------------------------------------------------------------------------------
struct CompositeBwdArgs {
  const float* deltas;   // [rays, S]
  const float* steps;    // [rays, S] sample mid-points t (only read with g_depth)
  const float* sigma;    // [rays, S]
  const float* color;    // [rays, S, 3] or NULL
  const float* g_w;      // [rays, S] or NULL
  const float* g_rgb;    // [rays, 3] or NULL
  const float* g_depth;  // [rays] or NULL (gradient w.r.t. the UN-clipped depth)
  int rays, samples;
  float* g_sigma;        // [rays, S]
  float* g_color;        // [rays, S, 3] or NULL
};

// The arithmetic is float64 on the fp32 inputs, rounded once at the store.  In fp32 the kernel met the 2e-5 of
// test_composite_backward_equals_autograd, but not what tests/test_sampler_chain_gpu.py holds a ray's gradient to (a few ulps of
// its largest element, norm-wise per ray), for three reasons it measured one after the other:
//  * the depth in front of a sample taken as `inclusive scan - ds`: behind thin fog a dense sample kept 2^-24 (excl + ds) of error in
//    excl, i.e. that much RELATIVE error in its weight -- the largest of the ray (1.5e-3 at ds = 1e5, and in g_sigma of everything in
//    front of it).  It is the SHIFTED scan now, as in tile_weights;
//  * the suffix sums taken as `tile sum - inclusive prefix`: 2^-24 of the tile's sum in every lane, 4 x the gradients behind a first
//    sample with ds = 16 (they are exp(-excl) small).  They are scanned from the far end of the tile now;
//  * dL/dds_k = G_k T_{k+1} - sum_{s>k} G_s w_s cancels (10 x where the next samples absorb most of the ray): an ulp each in ds, T, w
//    and G left 8.4e-7 of a ray's gradient against the 6.6e-7 allowed, with nothing wrong in any single step.  Hence float64:
//    3 exp + 1 expm1 per sample, in a kernel that took 0.02 % of a perception training step in fp32
//    (profiles/r04_train_perception_kernel_stats.csv).
__device__ __forceinline__ double wave_incl_scan(double v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}
// inclusive scan from the last lane towards this one
__device__ __forceinline__ double wave_incl_suffix_scan(double v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_down(v, o, 64);
    if (lane + o < 64) v += t;
  }
  return v;
}
// the scan of the lanes in front of this one: the inclusive scan shifted by a lane (NOT `incl - v`, see above)
__device__ __forceinline__ double shifted_scan(double incl, int lane) {
  const double t = __shfl_up(incl, 1, 64);
  return lane == 0 ? 0.0 : t;
}

#define NJF_COMPOSITE_MAX_TILES 16  // 1,024 samples per ray

__global__ void __launch_bounds__(256) composite_backward_kernel(CompositeBwdArgs a) {
  __shared__ double tile_start[4][NJF_COMPOSITE_MAX_TILES];  // per wave: optical depth in front of each 64-sample tile
  const int ray = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool live = ray < a.rays;
  const int S = a.samples, tiles = (S + 63) >> 6;
  const size_t base = (size_t)min(ray, a.rays - 1) * S;
  // forward sweep: the optical depth in front of every tile (accumulated front to back, like the forward pass -- taking it
  // from the ray's total by subtraction loses 1e-4 of the transmittance on opaque rays), sum w and sum w t (depth)
  double sum_w = 0.0, sum_wt = 0.0, carry = 0.0;
  const bool need_depth = a.g_depth != nullptr;
  for (int t = 0; t < tiles; ++t) {
    const int s = t * 64 + lane;
    const bool valid = s < S;
    const float delta = valid ? a.deltas[base + s] : 0.f;
    const double ds = (valid && delta > 0.f) ? (double)delta * (double)a.sigma[base + s] : 0.0;
    const double incl = wave_incl_scan(ds, lane);
    if (lane == 0) tile_start[wv][t] = carry;
    if (need_depth) {
      const double w = -expm1(-ds) * exp(-(carry + shifted_scan(incl, lane)));
      sum_w += valid ? w : 0.0;
      sum_wt += valid ? w * (double)a.steps[base + s] : 0.0;
    }
    carry += __shfl(incl, 63, 64);
  }
  if (need_depth) {
    sum_w = wave_sum(sum_w);
    sum_wt = wave_sum(sum_wt);
  }
  __syncthreads();  // tile_start written by lane 0 of each wave, read by all of its lanes (uniform trip counts: S is per launch)
  if (!live) return;
  const double denom = sum_w + 1e-10;
  const double depth = sum_wt / denom;
  const double gd = need_depth ? (double)a.g_depth[ray] / denom : 0.0;
  double gr[3] = {0.0, 0.0, 0.0};
  if (a.g_rgb) {
    gr[0] = a.g_rgb[3 * (size_t)ray];
    gr[1] = a.g_rgb[3 * (size_t)ray + 1];
    gr[2] = a.g_rgb[3 * (size_t)ray + 2];
  }
  double behind = 0.0;   // sum of G_s w_s over the tiles already visited (samples further along the ray)
  for (int t = tiles - 1; t >= 0; --t) {
    const int s = t * 64 + lane;
    const bool valid = s < S;
    const float delta = valid ? a.deltas[base + s] : 0.f;
    const double ds = (valid && delta > 0.f) ? (double)delta * (double)a.sigma[base + s] : 0.0;
    const double incl = wave_incl_scan(ds, lane);
    const double before = tile_start[wv][t];            // optical depth in front of this tile
    const double t_next = exp(-(before + incl));        // T_{s+1}
    const double w = -expm1(-ds) * exp(-(before + shifted_scan(incl, lane)));
    double G = a.g_w ? (valid ? (double)a.g_w[base + s] : 0.0) : 0.0;
    if (a.color && valid) {
      G += gr[0] * (double)a.color[3 * (base + s)] + gr[1] * (double)a.color[3 * (base + s) + 1] +
           gr[2] * (double)a.color[3 * (base + s) + 2];
    }
    if (need_depth && valid) G += gd * ((double)a.steps[base + s] - depth);
    const double gw = valid ? G * w : 0.0;
    // exclusive suffix sum inside the tile, scanned from the far end
    const double post = wave_incl_suffix_scan(gw, lane);
    const double tile_gw = __shfl(post, 0, 64);
    const double after = __shfl_down(post, 1, 64);
    const double suffix = behind + (lane == 63 ? 0.0 : after);
    if (valid) {
      a.g_sigma[base + s] = delta > 0.f ? (float)((double)delta * (G * t_next - suffix)) : 0.f;
      if (a.g_color) {
        a.g_color[3 * (base + s)] = (float)(w * gr[0]);
        a.g_color[3 * (base + s) + 1] = (float)(w * gr[1]);
        a.g_color[3 * (base + s) + 2] = (float)(w * gr[2]);
      }
    }
    behind += tile_gw;
  }
}

extern "C" int njf_composite_backward(const float* deltas, const float* steps, const float* sigma, const float* color,
                                      const float* g_weights, const float* g_rgb, const float* g_depth, int rays, int samples,
                                      float* g_sigma, float* g_color, void* stream) {
  if (!deltas || !sigma || !g_sigma) return NJF_E_NULL;
  if (g_depth && !steps) return NJF_E_NULL;
  if ((g_rgb || g_color) && !color) return NJF_E_NULL;
  if (rays < 1 || samples < 1) return NJF_E_SHAPE;
  if (samples > 64 * NJF_COMPOSITE_MAX_TILES) return NJF_E_SAMPLES;
  CompositeBwdArgs a{deltas, steps, sigma, color, g_weights, g_rgb, g_depth, rays, samples, g_sigma, g_color};
  composite_backward_kernel<<<(rays + 3) / 4, 256, 0, (hipStream_t)stream>>>(a);
  return launch_status();
}

struct PdfArgs {
  const float* weights;
  const float* bins_in;
  int bins_per_ray, s_in;
  const float* u;
  int u_per_ray, s_out;
  float anneal;
  int rays;
  float* bins_out;
};

__global__ void __launch_bounds__(NJF_THREADS) pdf_kernel(PdfArgs a) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int ray = blockIdx.x * NJF_WAVES + wave;
  const bool ok = ray < a.rays;
  const int rayc = min(ray, a.rays - 1);
  float* sc = njf_lds + LDS_SCRATCH_PROPOSAL + wave * LDS_SCRATCH_PER_WAVE;
  for (int s = lane; s < a.s_in; s += 64) {
    float w = a.weights[(size_t)rayc * a.s_in + s];
    if (a.anneal != 1.0f) w = powf(w, a.anneal);
    sc[s] = w + 0.01f;
  }
  __syncthreads();
  const float* bins = a.bins_in + (a.bins_per_ray ? (size_t)rayc * (a.s_in + 1) : 0);
  const float* u = a.u + (a.u_per_ray ? (size_t)rayc * (a.s_out + 1) : 0);
  pdf_resample_ray(sc, bins, a.s_in, u, a.s_out, a.bins_out + (size_t)rayc * (a.s_out + 1), lane, ok);
}

extern "C" int njf_pdf_resample(const float* weights, const float* bins_in, int bins_per_ray, int s_in, const float* u,
                                int u_per_ray, int s_out, float anneal, int rays, float* bins_out, void* stream) {
  if (!weights || !bins_in || !u || !bins_out) return NJF_E_NULL;
  if (rays < 1 || s_out < 1) return NJF_E_SHAPE;
  if (s_in < 1 || s_in > 256) return NJF_E_SAMPLES;
  PdfArgs a{weights, bins_in, bins_per_ray, s_in, u, u_per_ray, s_out, anneal, rays, bins_out};
  pdf_kernel<<<(rays + NJF_WAVES - 1) / NJF_WAVES, NJF_THREADS, LDS_FLOATS_PROPOSAL * sizeof(float), (hipStream_t)stream>>>(a);
  return launch_status();
}

// =============================================================================================
// launchers of the fused kernels
// =============================================================================================
static int check_common(const float* origins, const float* directions, int rays_per_batch, const NjfCameras* cams,
                        const NjfFeatureMap* gmap) {
  if (!origins || !directions || !cams || !gmap) return NJF_E_NULL;
  if (!cams->ctxt_w2c || !cams->ctxt_k || !cams->z_near || !cams->z_far || !gmap->data) return NJF_E_NULL;
  if (rays_per_batch < 1 || cams->batch < 1 || gmap->height < 1 || gmap->width < 1) return NJF_E_SHAPE;
  if ((long long)rays_per_batch * cams->batch > 0x7fffffffLL / 64) return NJF_E_SHAPE;
  if ((long long)gmap->height * gmap->width * gmap->stride > 0x7fffffffLL) return NJF_E_SHAPE;  // texel offsets are int32
  return NJF_OK;
}

// `precision`: of the network that reads the block (a plain-fp16 network reads a map of halves: 16-byte pieces = 8 elements)
static int check_gmap(const NjfFeatureMap* gmap, int off, int channels = NJF_ZDIM, int precision = NJF_PRECISION_F32) {
  const int mask = precision == NJF_PRECISION_F16 ? 7 : 3;
  if (off < 0 || (off & mask) || (gmap->stride & mask) || off + channels > gmap->stride) return NJF_E_GMAP;
  return NJF_OK;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is needed once per (kernel, device), not per launch: a lock-free
// set of the function pointers already raised, per device (every fused kernel is always launched with the same LDS size).
static std::atomic<const void*> g_lds_raised[16][256];

static bool lds_attribute_known(const void* fn) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return false;
  const size_t h = ((uintptr_t)fn >> 4) & 255;
  for (int i = 0; i < 256; ++i) {
    const void* v = g_lds_raised[dev][(h + i) & 255].load(std::memory_order_acquire);
    if (v == fn) return true;
    if (v == nullptr) return false;
  }
  return false;
}

static void lds_attribute_remember(const void* fn) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return;
  const size_t h = ((uintptr_t)fn >> 4) & 255;
  for (int i = 0; i < 256; ++i) {
    const void* expected = nullptr;
    std::atomic<const void*>& slot = g_lds_raised[dev][(h + i) & 255];
    if (slot.compare_exchange_strong(expected, fn, std::memory_order_acq_rel) || expected == fn) return;
  }
}

#ifdef NJF_STAMPS
extern "C" int njf_debug_read_stamps(unsigned* host_out, int n) {
  if (n > NJF_STAMP_SLOTS) n = NJF_STAMP_SLOTS;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(njf_stamp_out), (size_t)n * sizeof(unsigned));
}
#endif

template <typename K, typename A, typename... More>
static int launch_fused(K kernel, const A& args, int work_items, hipStream_t s, int lds_floats = LDS_FLOATS_RENDER,
                        const More&... more) {
  static_assert(sizeof(A) + (sizeof(More) + ... + 0) <= 4096, "kernel args too large");
  const int grid = (work_items + NJF_WAVES - 1) / NJF_WAVES;
#ifdef NJF_STAMPS
  const size_t lds = (size_t)(lds_floats + NJF_STAMP_SLOTS) * sizeof(float);
#else
  const size_t lds = (size_t)lds_floats * sizeof(float);
#endif
  if (!lds_attribute_known((const void*)kernel)) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    lds_attribute_remember((const void*)kernel);
  }
  kernel<<<grid, NJF_THREADS, lds, s>>>(args, more...);
  return launch_status();
}

// run `f(std::integral_constant<int, PREC_*>)` for the MFMA precision selected at run time.  TRAIN: the dispatch of the
// training forwards (activation dumps), which do not exist in the plain-fp16 mode -- NJF_E_MODE there.
template <bool TRAIN = false, typename F>
static int with_precision(int precision, F&& f) {
#ifdef NJF_DEV_ONLY_PREC  // development builds only (static ISA checks of one precision: a third of the compile time)
  if constexpr (TRAIN && NJF_DEV_ONLY_PREC == PREC_F16) return NJF_E_MODE;
  else return f(std::integral_constant<int, NJF_DEV_ONLY_PREC>{});
#else
  if (precision == NJF_PRECISION_F16X2) return f(std::integral_constant<int, PREC_F16X2>{});
  if (precision == NJF_PRECISION_F16F6) return f(std::integral_constant<int, PREC_F16F6>{});
  if (precision == NJF_PRECISION_F16) {
    if constexpr (TRAIN) return NJF_E_MODE;
    else return f(std::integral_constant<int, PREC_F16>{});
  }
  return f(std::integral_constant<int, PREC_F32>{});
#endif
}
// ... and `f(P_density, P_jacobian)` for the decoder kernels, whose Jacobian head may run in the other split precision
template <bool TRAIN = false, typename F>
static int with_precisions(int precision, F&& f) {
  const int d = density_precision(precision), j = jacobian_precision(precision);
#ifdef NJF_DEV_ONLY_PREC
  return with_precision<TRAIN>(d, [&](auto P) { return f(P, P); });
#else
  if (d == j) return with_precision<TRAIN>(d, [&](auto P) { return f(P, P); });
  if (d == NJF_PRECISION_F16F6) return f(std::integral_constant<int, PREC_F16F6>{}, std::integral_constant<int, PREC_F16X2>{});
  return f(std::integral_constant<int, PREC_F16X2>{}, std::integral_constant<int, PREC_F16F6>{});
#endif
}
#define NJF_P decltype(P)::value
#define NJF_PJ decltype(PJ)::value

extern "C" int njf_proposal_forward(const float* origins, const float* directions, int rays_per_batch,
                                    const NjfCameras* cams, const NjfFeatureMap* gmap, int gmap_offset,
                                    const float* w_pack, const float* b_pack, const float* bins_in, int bins_per_ray,
                                    int s_in, const float* u, int u_per_ray, int s_out, float anneal, float* bins_out,
                                    float* weights_out, float* density_out, const NjfActivationDump* dump,
                                    int precision, void* stream) {
  int rc = check_common(origins, directions, rays_per_batch, cams, gmap);
  if (rc) return rc;
  if (!w_pack || !b_pack || !bins_in || !u || !bins_out) return NJF_E_NULL;
  if (s_in < 1 || s_in > 256 || s_out < 1) return NJF_E_SAMPLES;
  if (!valid_base_precision(precision)) return NJF_E_MODE;
  if ((rc = check_gmap(gmap, gmap_offset, NJF_ZDIM, precision))) return rc;
  ProposalArgs a;
  a.rc = RayCommon{origins, directions, rays_per_batch, rays_per_batch * cams->batch, *cams, *gmap};
  a.gmap_offset = gmap_offset;
  a.w_pack = w_pack;
  a.b_pack = b_pack;
  a.bins_in = bins_in;
  a.bins_per_ray = bins_per_ray;
  a.s_in = s_in;
  a.u = u;
  a.u_per_ray = u_per_ray;
  a.s_out = s_out;
  a.anneal = anneal;
  a.bins_out = bins_out;
  a.weights_out = weights_out;
  a.density_out = density_out;
  a.dump = NjfActivationDump{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
  if (dump != nullptr && dump->act != nullptr) {  // training forward: inputs of the proposal net's backward pass
    if (!dump->pe || !dump->foot_idx || !dump->foot_w) return NJF_E_NULL;
    a.dump = *dump;
    return with_precision<true>(precision, [&](auto P) {
      return launch_fused(proposal_kernel<NJF_P, true>, a, a.rc.total_rays, (hipStream_t)stream, LDS_FLOATS_PROPOSAL);
    });
  }
  return with_precision(precision, [&](auto P) {
    return launch_fused(proposal_kernel<NJF_P>, a, a.rc.total_rays, (hipStream_t)stream, LDS_FLOATS_PROPOSAL);
  });
}

// The decoder blobs must be one allocation laid out [density | colour | jacobian] (what
// njf_pack_* write when given consecutive destinations); the launcher verifies contiguity.
static int check_jacobian(int kind, const NjfCameras* cams, const NjfFeatureMap* gmap, int goff_j, const float* w_j,
                          const float* b_j, int precision) {
  if (kind == NJF_JACOBIAN_NONE) return NJF_OK;
  if (kind != NJF_JACOBIAN_MLP && kind != NJF_JACOBIAN_TRANSFORMER) return NJF_E_MODE;
  if (!w_j || !b_j) return NJF_E_NULL;
  const int max_a = kind == NJF_JACOBIAN_MLP ? NJF_MAX_ACTION_DIM : 8;  // transformer: 8 key slots per head
  if (cams->action_dim < 1 || cams->action_dim > max_a) return NJF_E_ACTION_DIM;
  return check_gmap(gmap, goff_j, kind == NJF_JACOBIAN_MLP ? NJF_ZDIM : NJF_QDIM, jacobian_precision(precision));
}

static int check_contiguous(const float* w_d, const float* w_c, const float* w_j, bool with_j) {
  if (w_c != w_d + NJF_RESNET_W_FLOATS) return NJF_E_SHAPE;
  if (with_j && w_j != w_c + NJF_COLOR_W_FLOATS) return NJF_E_SHAPE;
  return NJF_OK;
}

extern "C" int njf_render_forward(const float* origins, const float* directions, int rays_per_batch,
                                  const NjfCameras* cams, const NjfFeatureMap* gmap, int gmap_offset_density,
                                  int gmap_offset_jacobian, int jacobian_kind, const float* w_density,
                                  const float* b_density, const float* w_color, const float* b_color,
                                  const float* w_jacobian, const float* b_jacobian, const float* bins, int samples,
                                  const NjfRenderOutputs* out, int precision, void* stream) {
  int rc = check_common(origins, directions, rays_per_batch, cams, gmap);
  if (rc) return rc;
  if (!w_density || !b_density || !w_color || !b_color || !bins || !out) return NJF_E_NULL;
  if (samples < 1) return NJF_E_SAMPLES;
  if (!valid_precision(precision)) return NJF_E_MODE;
  if ((rc = check_gmap(gmap, gmap_offset_density, NJF_ZDIM, density_precision(precision)))) return rc;
  if ((rc = check_jacobian(jacobian_kind, cams, gmap, gmap_offset_jacobian, w_jacobian, b_jacobian, precision))) return rc;
  const bool with_j = jacobian_kind != NJF_JACOBIAN_NONE;
  if ((rc = check_contiguous(w_density, w_color, w_jacobian, with_j))) return rc;
  RenderArgs a;
  a.rc = RayCommon{origins, directions, rays_per_batch, rays_per_batch * cams->batch, *cams, *gmap};
  a.goff_d = gmap_offset_density;
  a.goff_j = with_j ? gmap_offset_jacobian : gmap_offset_density;
  a.w_all = w_density;
  a.b_d = b_density;
  a.b_c = b_color;
  a.b_j = b_jacobian;
  a.bins = bins;
  a.samples = samples;
  a.out = *out;
  hipStream_t s = (hipStream_t)stream;
  const int n = a.rc.total_rays;
  // Training forwards keep the AF = true instantiations (the 16 action-feature accumulators stay allocated although no training
  // forward composites them any more, model.py::_vis_at_bins).  Round 5 built the AF = false ones to get the dump kernels off the
  // spill path -- 104-119 spilled VGPRs -> 45-68 -- and measured them SLOWER or equal on the C4 shard (1 x 8,192 rays: action step
  // 8.56 vs 8.34 ms, perception 13.63 vs 13.67 ms, two repetitions each, profiles/r05_spills_ab.txt): the spills are not what
  // these kernels wait for.  -DNJF_TRAIN_NO_AF rebuilds the A/B.
  constexpr bool TRAIN_AF = true;
  const bool training_forward = out->jac_act != nullptr || out->jac_pe != nullptr || out->den_act != nullptr;
  if (!TRAIN_AF && training_forward && out->action_features != nullptr) return NJF_E_MODE;
  if (out->jac_act != nullptr || (out->jac_pe != nullptr && out->den_act == nullptr)) {
    // action-mode training forward: dump the Jacobian head's backward-pass inputs (ResnetFC head: activations +
    // encoding + footprint; transformer head: encoding + footprint, the head is recomputed by the backward pass)
    if (jacobian_kind == NJF_JACOBIAN_NONE || out->den_act) return NJF_E_MODE;
    if (!out->jac_pe || !out->foot_idx || !out->foot_w) return NJF_E_NULL;
    if (jacobian_kind == NJF_JACOBIAN_MLP) {
      if (!out->jac_act) return NJF_E_NULL;
      return with_precisions<true>(precision, [&](auto P, auto PJ) { return launch_fused(render_kernel<1, NJF_P, 1, TRAIN_AF, NJF_PJ>, a, n, s); });
    }
    // (transformer head: jac_act is optional and has another shape, [4, P, 64]: the residual stream njf_transformer_backward reads)
    if (out->dump_f16 || out->jac_mask) return NJF_E_MODE;
    return with_precisions<true>(precision, [&](auto P, auto PJ) { return launch_fused(render_kernel<2, NJF_P, 1, TRAIN_AF, NJF_PJ>, a, n, s); });
  }
  if (out->den_act != nullptr) {  // perception-mode training forward: dump the density net and the colour head
    if (!out->jac_pe || !out->foot_idx || !out->foot_w || !out->col_in || !out->col_act) return NJF_E_NULL;
    if (jacobian_kind == NJF_JACOBIAN_NONE)
      return with_precision<true>(density_precision(precision), [&](auto P) { return launch_fused(render_kernel<0, NJF_P, 2, TRAIN_AF>, a, n, s); });
    return with_precisions<true>(precision, [&](auto P, auto PJ) {
      if (jacobian_kind == NJF_JACOBIAN_MLP) return launch_fused(render_kernel<1, NJF_P, 2, TRAIN_AF, NJF_PJ>, a, n, s);
      return launch_fused(render_kernel<2, NJF_P, 2, TRAIN_AF, NJF_PJ>, a, n, s);
    });
  }
  const bool af = with_j && out->action_features != nullptr;
  if (jacobian_kind == NJF_JACOBIAN_NONE)
    return with_precision(density_precision(precision), [&](auto P) { return launch_fused(render_kernel<0, NJF_P, 0, false>, a, n, s); });
  return with_precisions(precision, [&](auto P, auto PJ) {
    if (jacobian_kind == NJF_JACOBIAN_MLP)
      return af ? launch_fused(render_kernel<1, NJF_P, 0, true, NJF_PJ>, a, n, s) : launch_fused(render_kernel<1, NJF_P, 0, false, NJF_PJ>, a, n, s);
    return af ? launch_fused(render_kernel<2, NJF_P, 0, true, NJF_PJ>, a, n, s) : launch_fused(render_kernel<2, NJF_P, 0, false, NJF_PJ>, a, n, s);
  });
}

// ---- the decoder at points (points_kernel): what its three entry points share ----------------------------------------------
// Validation and the shared kernel arguments; returns the evaluator's MODE, or an error (< 0).  mode 0: the proposal net; mode 1:
// the decoder, of which `density_only` (no Jacobian head asked for either) runs the density net alone.  The outputs are the caller's.
static int make_decoder_args(const NjfCameras* cams, const NjfFeatureMap* gmap, int gmap_offset_density, int gmap_offset_jacobian,
                             int mode, int jacobian_kind, bool density_only, const float* w_density, const float* b_density,
                             const float* w_color, const float* b_color, const float* w_jacobian, const float* b_jacobian,
                             int precision, DecoderArgs& a) {
  if (!cams || !gmap || !w_density || !b_density) return NJF_E_NULL;
  if (!cams->ctxt_w2c || !cams->ctxt_k || !gmap->data) return NJF_E_NULL;
  if (cams->batch < 1) return NJF_E_SHAPE;
  if (mode != 0 && mode != 1) return NJF_E_MODE;
  if (!valid_precision(precision)) return NJF_E_MODE;
  if (gmap->height < 1 || gmap->width < 1) return NJF_E_SHAPE;
  int rc;
  if ((rc = check_gmap(gmap, gmap_offset_density, NJF_ZDIM, density_precision(precision)))) return rc;
  // a point carries the float index of its batch element in 32 bits (PointGeom::gofs): maps up to 16 GiB
  if ((long long)cams->batch * gmap->height * gmap->width * gmap->stride > 0xffffffffLL) return NJF_E_SHAPE;
  int kmode = 0;
  if (mode == 1) {
    if ((rc = check_jacobian(jacobian_kind, cams, gmap, gmap_offset_jacobian, w_jacobian, b_jacobian, precision))) return rc;
    const bool with_j = jacobian_kind != NJF_JACOBIAN_NONE;
    static_assert(NJF_JACOBIAN_MLP == 1 && NJF_JACOBIAN_TRANSFORMER == 2, "MODE 3 / 4 = 2 + the head's kind");
    kmode = !with_j && density_only ? 1 : 2 + jacobian_kind;
    if (kmode >= 2) {
      if (!w_color || !b_color) return NJF_E_NULL;
      if ((rc = check_contiguous(w_density, w_color, w_jacobian, with_j))) return rc;
    }
  }
  a = DecoderArgs{*cams, *gmap, gmap_offset_density, gmap_offset_jacobian, w_density, b_density, b_color, b_jacobian};
  return kmode;
}

// the one dispatch on (MODE, precisions, FEAT): a source has the instantiations of its SRC::MODES, the feature dump those of
// the point list's ResnetFC head
template <int MODE, class SRC>
static int launch_points_mode(const SRC& src, const DecoderArgs& a, int tiles, int precision, hipStream_t s) {
  auto launch = [&](auto kernel) { return launch_fused(kernel, a, tiles, s, LDS_FLOATS_RENDER, src); };
  if constexpr (!((SRC::MODES >> MODE) & 1)) return NJF_E_MODE;
  else if constexpr (MODE <= 2)
    return with_precision(density_precision(precision), [&](auto P) { return launch(points_kernel<SRC, MODE, NJF_P>); });
  else
    return with_precisions(precision, [&](auto P, auto PJ) {
      if constexpr (MODE == 3 && SRC::EXTRAS) {
        if (a.features) {  // (the plain-fp16 mode has no training instantiation of resnet_tile: its block biases ride elsewhere)
          if constexpr (NJF_PJ == PREC_F16) return (int)NJF_E_MODE;
          else return launch(points_kernel<SRC, 3, NJF_P, NJF_PJ, true>);
        }
      }
      return launch(points_kernel<SRC, MODE, NJF_P, NJF_PJ>);
    });
}

template <class SRC>
static int launch_points(const SRC& src, const DecoderArgs& a, int kmode, int entries, int precision, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int tiles = (entries + 31) / 32;
  switch (kmode) {
    case 0: return launch_points_mode<0>(src, a, tiles, precision, s);
    case 1: return launch_points_mode<1>(src, a, tiles, precision, s);
    case 2: return launch_points_mode<2>(src, a, tiles, precision, s);
    case 3: return launch_points_mode<3>(src, a, tiles, precision, s);
    default: return launch_points_mode<4>(src, a, tiles, precision, s);
  }
}

static ConstantDirection view_direction(const float* view_dir) {
  return view_dir ? ConstantDirection{view_dir[0], view_dir[1], view_dir[2]} : ConstantDirection{0.f, 0.f, 1.f};
}

extern "C" int njf_points_forward(const float* xyz, const float* dirs, int points_per_batch, const NjfCameras* cams,
                                  const NjfFeatureMap* gmap, int gmap_offset_density, int gmap_offset_jacobian, int mode,
                                  int jacobian_kind, const float* w_density, const float* b_density, const float* w_color,
                                  const float* b_color, const float* w_jacobian, const float* b_jacobian, float* density,
                                  float* color, float* flow, float* jacobian, float* geo, float* features, int precision,
                                  void* stream) {
  if (!xyz) return NJF_E_NULL;
  if (points_per_batch < 1) return NJF_E_SHAPE;
  DecoderArgs a;
  const int kmode = make_decoder_args(cams, gmap, gmap_offset_density, gmap_offset_jacobian, mode, jacobian_kind, false, w_density,
                                      b_density, w_color, b_color, w_jacobian, b_jacobian, precision, a);
  if (kmode < 0) return kmode;
  const PointList src{xyz, dirs, points_per_batch, points_per_batch * cams->batch};
  // the per-block features exist for a ResnetFC head evaluated next to the decoder (mode 1, NJF_JACOBIAN_MLP)
  if (features && kmode != 3) return NJF_E_MODE;
  if (features && (long long)src.total * 5 * 128 > 0x7fffffffffLL) return NJF_E_SHAPE;
  a.density = density, a.color = color, a.jacobian = jacobian, a.flow = flow, a.geo = geo, a.features = features;
  return launch_points(src, a, kmode, src.total, precision, stream);
}

// ---- voxel-grid field extraction ---------------------------------------------------------------------------------
static int make_field_list(const NjfFieldGrid* grid, int batch, const int* indices, const int* count, int capacity,
                           FieldList& l) {
  if (!grid) return NJF_E_NULL;
  if (batch < 1 || capacity < 0) return NJF_E_SHAPE;
  long long total = batch;
  for (int c = 0; c < 3; ++c) {
    if (grid->dims[c] < 1) return NJF_E_SHAPE;
    total *= grid->dims[c];
    if (total > 0x7fffffffLL) return NJF_E_SHAPE;  // global indices are int32: B*N < 2^31
  }
  if (!indices && capacity > total) return NJF_E_SHAPE;  // the identity list has B*N entries
  l.grid = *grid;
  l.total = (int)total;
  l.nodes = l.total / batch;
  l.indices = indices;
  l.count = count;
  l.capacity = capacity;
  return NJF_OK;
}

extern "C" int njf_field_points(const NjfFieldGrid* grid, int batch, const int* indices, const int* count, int capacity,
                                float* xyz, void* stream) {
  FieldList l;
  int rc = make_field_list(grid, batch, indices, count, capacity, l);
  if (rc) return rc;
  if (!xyz) return NJF_E_NULL;
  if (capacity == 0) return NJF_OK;
  field_xyz_kernel<<<(capacity + 255) / 256, 256, 0, (hipStream_t)stream>>>(l, xyz);
  return launch_status();
}

extern "C" int njf_field_select(const NjfFieldGrid* grid, const NjfCameras* cams, int batch, const float* values,
                                float threshold, const int* indices, const int* count, int capacity, int* out_indices,
                                int* out_count, int out_capacity, int* workspace, void* stream) {
  SelectArgs a;
  int rc = make_field_list(grid, batch, indices, count, capacity, a.list);
  if (rc) return rc;
  if (!out_count || !workspace || (!values && !cams)) return NJF_E_NULL;  // (no predicate: nothing to select)
  if (out_capacity < 0 || (out_capacity > 0 && !out_indices)) return out_capacity < 0 ? NJF_E_SHAPE : NJF_E_NULL;
  if (cams && (!cams->ctxt_w2c || !cams->ctxt_k)) return NJF_E_NULL;
  if (cams && cams->batch != batch) return NJF_E_SHAPE;
  a.values = values;
  a.threshold = threshold;
  a.w2c = cams ? cams->ctxt_w2c : nullptr;
  a.k = cams ? cams->ctxt_k : nullptr;
  a.out_indices = out_indices;
  a.out_count = out_count;
  a.out_capacity = out_capacity;
  a.block_counts = workspace;
  a.blocks = (int)(((long long)capacity + NJF_FIELD_SELECT_BLOCK - 1) / NJF_FIELD_SELECT_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  if (a.blocks > 0) {
    select_count_kernel<<<a.blocks, NJF_BLOCK_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  block_offsets_kernel<1><<<1, NJF_BLOCK_THREADS, 0, s>>>(workspace, a.blocks, out_count);
  if ((rc = launch_status())) return rc;
  if (a.blocks > 0 && out_capacity > 0) {
    select_scatter_kernel<<<a.blocks, NJF_BLOCK_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  return NJF_OK;
}

extern "C" int njf_field_forward(const NjfFieldGrid* grid, const int* indices, const int* count, int capacity,
                                 const float* view_dir, const NjfCameras* cams, const NjfFeatureMap* gmap,
                                 int gmap_offset_density, int gmap_offset_jacobian, int mode, int jacobian_kind,
                                 const float* w_density, const float* b_density, const float* w_color, const float* b_color,
                                 const float* w_jacobian, const float* b_jacobian, float* density, float* color,
                                 float* jacobian, int precision, void* stream) {
  if (!grid || !cams) return NJF_E_NULL;
  GridNodes src{view_direction(view_dir)};
  int rc = make_field_list(grid, cams->batch, indices, count, capacity, src.list);
  if (rc) return rc;
  DecoderArgs a;  // (no head and no colour output: the density net's blob is all that is streamed)
  const int kmode = make_decoder_args(cams, gmap, gmap_offset_density, gmap_offset_jacobian, mode, jacobian_kind, !color, w_density,
                                      b_density, w_color, b_color, w_jacobian, b_jacobian, precision, a);
  if (kmode < 0) return kmode;
  if (kmode <= 1 ? !density : (kmode == 2 ? !color : !jacobian)) return NJF_E_NULL;  // the last stage's output
  a.density = density, a.color = color, a.jacobian = jacobian;
  if (capacity == 0) return NJF_OK;
  return launch_points(src, a, kmode, capacity, precision, stream);
}

// ---- isosurface mesh ---------------------------------------------------------------------------------------------------
static int make_mesh_args(const NjfFieldGrid* grid, const NjfCameras* cams, int batch, const float* values,
                          const unsigned char* valid, float threshold, int phase, unsigned char* edge_mask, int* vertex_offset,
                          int* workspace, MeshArgs& a) {
  if (!grid || !values || !edge_mask || !vertex_offset || !workspace) return NJF_E_NULL;
  int rc = make_field_list(grid, batch, nullptr, nullptr, 0, a.sel.list);
  if (rc) return rc;
  if (grid->dims[0] < 2 || grid->dims[1] < 2 || grid->dims[2] < 2) return NJF_E_VALUE;  // no cell
  if (!__builtin_isfinite(threshold)) return NJF_E_VALUE;
  if (phase < 1 || phase > 3) return NJF_E_VALUE;
  if (cams && (!cams->ctxt_w2c || !cams->ctxt_k)) return NJF_E_NULL;
  if (cams && cams->batch != batch) return NJF_E_SHAPE;
  a.sel.list.capacity = a.sel.list.total;
  a.sel.values = values;
  a.sel.threshold = threshold;
  a.sel.w2c = cams ? cams->ctxt_w2c : nullptr;
  a.sel.k = cams ? cams->ctxt_k : nullptr;
  a.sel.out_indices = nullptr;
  a.sel.out_count = nullptr;
  a.sel.out_capacity = 0;
  a.sel.block_counts = nullptr;
  a.sel.blocks = 0;
  a.valid = valid;
  a.mask = edge_mask;
  a.offset = vertex_offset;
  a.vertex_node = nullptr;
  a.vertex_edge = nullptr;
  a.vertex_t = nullptr;
  a.vertices = nullptr;
  a.max_vertices = 0;
  a.triangles = nullptr;
  a.triangle_cell = nullptr;
  a.max_triangles = 0;
  a.cells = (grid->dims[0] - 1) * (grid->dims[1] - 1) * (grid->dims[2] - 1);
  a.total_cells = batch * a.cells;
  a.block_counts = workspace;
  return NJF_OK;
}

extern "C" int njf_field_mesh_vertices(const NjfFieldGrid* grid, const NjfCameras* cams, int batch, const float* values,
                                       const unsigned char* valid, float threshold, int phase, unsigned char* edge_mask,
                                       int* vertex_offset, int* vertex_node, unsigned char* vertex_edge, float* vertex_t,
                                       float* vertices, int max_vertices, int* vertex_count, int* workspace, void* stream) {
  MeshArgs a;
  int rc = make_mesh_args(grid, cams, batch, values, valid, threshold, phase, edge_mask, vertex_offset, workspace, a);
  if (rc) return rc;
  if ((phase & NJF_FIELD_MESH_COUNT) && !vertex_count) return NJF_E_NULL;
  if (max_vertices < 0) return NJF_E_VALUE;
  if ((phase & NJF_FIELD_MESH_EMIT) && max_vertices > 0 && (!vertex_node || !vertex_edge || !vertex_t || !vertices)) return NJF_E_NULL;
  a.vertex_node = vertex_node;
  a.vertex_edge = vertex_edge;
  a.vertex_t = vertex_t;
  a.vertices = vertices;
  a.max_vertices = max_vertices;
  const int blocks = (int)(((long long)a.sel.list.total + NJF_FIELD_MESH_BLOCK - 1) / NJF_FIELD_MESH_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  if (phase & NJF_FIELD_MESH_COUNT) {
    mesh_mask_kernel<<<blocks, NJF_BLOCK_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
    block_offsets_kernel<1><<<1, NJF_BLOCK_THREADS, 0, s>>>(workspace, blocks, vertex_count);
    if ((rc = launch_status())) return rc;
  }
  if (phase & NJF_FIELD_MESH_EMIT) {
    mesh_vertex_kernel<<<blocks, NJF_BLOCK_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  return NJF_OK;
}

extern "C" int njf_field_mesh_triangles(const NjfFieldGrid* grid, int batch, const float* values, float threshold, int phase,
                                        const unsigned char* edge_mask, const int* vertex_offset, int* triangles,
                                        int* triangle_cell, int max_triangles, int* triangle_count, int* workspace,
                                        void* stream) {
  MeshArgs a;
  int rc = make_mesh_args(grid, nullptr, batch, values, nullptr, threshold, phase, const_cast<unsigned char*>(edge_mask),
                          const_cast<int*>(vertex_offset), workspace, a);
  if (rc) return rc;
  if ((phase & NJF_FIELD_MESH_COUNT) && !triangle_count) return NJF_E_NULL;
  if (max_triangles < 0) return NJF_E_VALUE;
  if ((phase & NJF_FIELD_MESH_EMIT) && max_triangles > 0 && (!triangles || !triangle_cell)) return NJF_E_NULL;
  a.triangles = triangles;
  a.triangle_cell = triangle_cell;
  a.max_triangles = max_triangles;
  const int blocks = (a.total_cells + NJF_FIELD_MESH_BLOCK - 1) / NJF_FIELD_MESH_BLOCK;
  hipStream_t s = (hipStream_t)stream;
  if (phase & NJF_FIELD_MESH_COUNT) {
    mesh_triangle_count_kernel<<<blocks, NJF_BLOCK_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
    block_offsets_kernel<1><<<1, NJF_BLOCK_THREADS, 0, s>>>(workspace, blocks, triangle_count);
    if ((rc = launch_status())) return rc;
  }
  if ((phase & NJF_FIELD_MESH_EMIT) && max_triangles > 0) {
    mesh_triangle_kernel<<<blocks, NJF_BLOCK_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  return NJF_OK;
}

extern "C" int njf_field_forward_at(const float* xyz, const int* node, const int* count, int capacity, int nodes_per_batch,
                                    const float* view_dir, const NjfCameras* cams, const NjfFeatureMap* gmap,
                                    int gmap_offset_density, int gmap_offset_jacobian, int jacobian_kind,
                                    const float* w_density, const float* b_density, const float* w_color, const float* b_color,
                                    const float* w_jacobian, const float* b_jacobian, float* density, float* color,
                                    float* jacobian, int precision, void* stream) {
  if (!xyz || !node || !cams) return NJF_E_NULL;
  if (capacity < 0) return NJF_E_SHAPE;
  if (nodes_per_batch < 1 || (long long)nodes_per_batch * cams->batch > 0x7fffffffLL) return NJF_E_VALUE;
  DecoderArgs a;
  const int kmode = make_decoder_args(cams, gmap, gmap_offset_density, gmap_offset_jacobian, 1, jacobian_kind, false, w_density,
                                      b_density, w_color, b_color, w_jacobian, b_jacobian, precision, a);
  if (kmode < 0) return kmode;
  if (kmode == 2 ? !color : !jacobian) return NJF_E_NULL;  // the last stage's output
  a.density = density, a.color = color, a.jacobian = jacobian;
  if (capacity == 0) return NJF_OK;
  const StoredNodes src{view_direction(view_dir), xyz, node, count, capacity, nodes_per_batch, nodes_per_batch * cams->batch};
  return launch_points(src, a, kmode, capacity, precision, stream);
}

// ---- fusion of several context views ----------------------------------------------------------------------------------
extern "C" int njf_field_fuse(const NjfFieldGrid* grid, const NjfCameras* cams, int scenes, int views, const float* values,
                              int mode, int min_views, float* fused, unsigned char* seen, unsigned char* valid, void* stream) {
  if (!grid || !values || !fused) return NJF_E_NULL;
  if (views < 1 || views > NJF_FIELD_MAX_VIEWS) return NJF_E_VALUE;
  if (min_views < 1 || min_views > views) return NJF_E_VALUE;
  if (mode != NJF_FIELD_FUSE_MEAN && mode != NJF_FIELD_FUSE_MIN && mode != NJF_FIELD_FUSE_MAX) return NJF_E_VALUE;
  if (scenes < 1 || scenes > 0x7fffffff / views) return NJF_E_SHAPE;
  FieldList l;
  int rc = make_field_list(grid, scenes * views, nullptr, nullptr, 0, l);  // G*V*N < 2^31
  if (rc) return rc;
  if (cams && (!cams->ctxt_w2c || !cams->ctxt_k)) return NJF_E_NULL;
  if (cams && cams->batch != scenes * views) return NJF_E_SHAPE;
  FuseArgs a;
  a.grid = *grid;
  a.nodes = l.nodes;
  a.views = views;
  a.blocks_per_scene = (l.nodes + NJF_FIELD_SELECT_BLOCK - 1) / NJF_FIELD_SELECT_BLOCK;
  a.min_views = min_views;
  a.w2c = cams ? cams->ctxt_w2c : nullptr;
  a.k = cams ? cams->ctxt_k : nullptr;
  a.values = values;
  a.fused = fused;
  a.seen = seen;
  a.valid = valid;
  const int blocks = scenes * a.blocks_per_scene;  // <= G*N
  hipStream_t s = (hipStream_t)stream;
  if (mode == NJF_FIELD_FUSE_MEAN) field_fuse_kernel<NJF_FIELD_FUSE_MEAN><<<blocks, NJF_BLOCK_THREADS, 0, s>>>(a);
  else if (mode == NJF_FIELD_FUSE_MIN) field_fuse_kernel<NJF_FIELD_FUSE_MIN><<<blocks, NJF_BLOCK_THREADS, 0, s>>>(a);
  else field_fuse_kernel<NJF_FIELD_FUSE_MAX><<<blocks, NJF_BLOCK_THREADS, 0, s>>>(a);
  return launch_status();
}

extern "C" int njf_field_combine(const float* xyz, const int* node, const int* count, int capacity, int nodes_per_scene,
                                 int views, const NjfCameras* cams, const float* density, const float* color,
                                 const float* jacobian, int action_dim, float* out_color, float* out_jacobian,
                                 unsigned char* out_views, void* stream) {
  if (views < 1 || views > NJF_FIELD_MAX_VIEWS || nodes_per_scene < 1) return NJF_E_VALUE;
  if (capacity < 0) return NJF_E_SHAPE;
  if ((color || jacobian) && !density) return NJF_E_NULL;
  if ((color && !out_color) || (jacobian && !out_jacobian)) return NJF_E_NULL;
  if (!color && !jacobian && !out_views) return NJF_E_NULL;  // (nothing to write)
  if (jacobian && (action_dim < 1 || action_dim > NJF_MAX_ACTION_DIM)) return NJF_E_ACTION_DIM;
  if (cams) {
    if (!cams->ctxt_w2c || !cams->ctxt_k || !xyz || !node) return NJF_E_NULL;
    if (cams->batch < views || cams->batch % views != 0) return NJF_E_SHAPE;
    if ((long long)(cams->batch / views) * nodes_per_scene > 0x7fffffffLL) return NJF_E_SHAPE;
  }
  CombineArgs a;
  a.xyz = xyz;
  a.node = node;
  a.count = count;
  a.capacity = capacity;
  a.nodes = nodes_per_scene;
  a.scenes = cams ? cams->batch / views : 1;
  a.views = views;
  a.w2c = cams ? cams->ctxt_w2c : nullptr;
  a.k = cams ? cams->ctxt_k : nullptr;
  a.density = (color || jacobian) ? density : nullptr;
  a.color = color;
  a.jacobian = jacobian;
  a.jdim = 3 * action_dim;
  a.out_color = out_color;
  a.out_jacobian = out_jacobian;
  a.out_views = out_views;
  if (capacity == 0) return NJF_OK;
  const int blocks = (int)(((long long)capacity + NJF_COMBINE_THREADS - 1) / NJF_COMBINE_THREADS);
  field_combine_kernel<<<blocks, NJF_COMBINE_THREADS, 0, (hipStream_t)stream>>>(a);
  return launch_status();
}

// ---- connected components of the inside nodes -----------------------------------------------------------------------------
extern "C" int njf_field_components(const NjfFieldGrid* grid, const NjfCameras* cams, int batch, const float* values,
                                    float threshold, const unsigned char* valid, const int* indices, const int* count,
                                    int capacity, const int* keys, int connectivity, int phase, int* labels, int* sizes,
                                    int* component_count, int* status, int* workspace, void* stream) {
  if (connectivity != 6 && connectivity != 14) return NJF_E_VALUE;
  if (phase < 1 || phase > NJF_FIELD_COMPONENTS_ALL) return NJF_E_VALUE;
  ComponentArgs a;
  int rc = make_field_list(grid, batch, nullptr, nullptr, 0, a.sel.list);
  if (rc) return rc;
  if (capacity < 0) return NJF_E_SHAPE;
  if ((values != nullptr) == (indices != nullptr)) return values ? NJF_E_VALUE : NJF_E_NULL;  // one form, not both
  if (indices && (valid || cams)) return NJF_E_VALUE;  // (a list IS the inside set)
  if (!labels || !sizes || !component_count || !status || !workspace) return NJF_E_NULL;
  if (cams && (!cams->ctxt_w2c || !cams->ctxt_k)) return NJF_E_NULL;
  if (cams && cams->batch != batch) return NJF_E_SHAPE;
  const int total = a.sel.list.total;
  a.sel.values = values;
  a.sel.threshold = threshold;
  a.sel.w2c = cams ? cams->ctxt_w2c : nullptr;
  a.sel.k = cams ? cams->ctxt_k : nullptr;
  a.sel.out_indices = nullptr;
  a.sel.out_count = nullptr;
  a.sel.out_capacity = 0;
  a.sel.block_counts = nullptr;
  a.sel.blocks = 0;
  a.valid = valid;
  a.entries = indices;
  a.entry_count = count;
  a.entry_capacity = capacity;
  a.keys = keys;
  a.dense_keys = !keys ? nullptr : (indices ? workspace + 2 * (size_t)total : const_cast<int*>(keys));
  a.half = connectivity / 2;
  a.parent = workspace;
  a.root_size = workspace + (size_t)total;
  a.labels = labels;
  a.sizes = sizes;
  a.count = component_count;
  a.status = status;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = (int)(((long long)total + NJF_FIELD_COMPONENTS_BLOCK - 1) / NJF_FIELD_COMPONENTS_BLOCK);
  if (phase & NJF_FIELD_COMPONENTS_INIT) {
    if (hipMemsetAsync(component_count, 0, sizeof(int), s) != hipSuccess) return launch_status();
    if (hipMemsetAsync(status, 0, sizeof(int), s) != hipSuccess) return launch_status();
    if (indices) components_init_kernel<true><<<blocks, NJF_CC_THREADS, 0, s>>>(a);
    else components_init_kernel<false><<<blocks, NJF_CC_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  if (phase & NJF_FIELD_COMPONENTS_MERGE) {
    components_merge_kernel<<<blocks, NJF_CC_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  if (phase & NJF_FIELD_COMPONENTS_LABEL) {
    components_label_kernel<<<blocks, NJF_CC_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  if (phase & NJF_FIELD_COMPONENTS_SIZES) {
    components_size_kernel<<<blocks, NJF_CC_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  return NJF_OK;
}

// ---- coarse-to-fine band ------------------------------------------------------------------------------------------------------
extern "C" int njf_field_band(const NjfFieldGrid* grid, int factor, int dilate, int batch, const float* coarse_values,
                              const unsigned char* coarse_valid, float coarse_threshold, unsigned char* block_active,
                              unsigned char* band, int* out_indices, int* out_count, int out_capacity, int* workspace,
                              void* stream) {
  if (!grid) return NJF_E_NULL;
  if (factor != 2 && factor != 4 && factor != 8 && factor != 16) return NJF_E_VALUE;
  if (dilate < 0 || dilate > 2) return NJF_E_VALUE;
  if (!__builtin_isfinite(coarse_threshold)) return NJF_E_VALUE;
  FieldList l;
  int rc = make_field_list(grid, batch, nullptr, nullptr, 0, l);
  if (rc) return rc;
  BandArgs a;
  a.shift = factor == 2 ? 1 : factor == 4 ? 2 : factor == 8 ? 3 : 4;
  for (int c = 0; c < 3; ++c) {
    if (grid->dims[c] < factor + 1 || (grid->dims[c] - 1) % factor != 0) return NJF_E_VALUE;
    a.dims[c] = grid->dims[c];
    a.m[c] = (grid->dims[c] - 1) / factor;
  }
  if (!coarse_values || !block_active || !band || !out_count || !workspace) return NJF_E_NULL;
  if (out_capacity < 0 || (out_capacity > 0 && !out_indices)) return out_capacity < 0 ? NJF_E_SHAPE : NJF_E_NULL;
  a.nodes = l.nodes;
  a.total = l.total;
  a.batch = batch;
  a.nb = a.m[0] * a.m[1] * a.m[2];
  a.dilate = dilate;
  a.cvalues = coarse_values;
  a.cvalid = coarse_valid;
  a.cthreshold = coarse_threshold;
  a.block_active = block_active;
  a.band = band;
  a.out_indices = out_indices;
  a.out_count = out_count;
  a.out_capacity = out_capacity;
  a.block_counts = workspace;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = (int)(((long long)a.total + NJF_FIELD_BAND_BLOCK - 1) / NJF_FIELD_BAND_BLOCK);
  band_blocks_kernel<<<(batch * a.nb + NJF_BLOCK_THREADS - 1) / NJF_BLOCK_THREADS, NJF_BLOCK_THREADS, 0, s>>>(a);
  if ((rc = launch_status())) return rc;
  band_count_kernel<<<blocks, NJF_BLOCK_THREADS, 0, s>>>(a);
  if ((rc = launch_status())) return rc;
  block_offsets_kernel<1><<<1, NJF_BLOCK_THREADS, 0, s>>>(workspace, blocks, out_count);
  if ((rc = launch_status())) return rc;
  if (out_capacity > 0) {
    band_scatter_kernel<<<blocks, NJF_BLOCK_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  return NJF_OK;
}

extern "C" int njf_field_scatter(const float* values, const int* indices, const int* count, int capacity, float* out,
                                 int out_size, void* stream) {
  if (capacity < 0 || out_size < 0) return NJF_E_SHAPE;
  if (capacity == 0) return NJF_OK;
  if (!values || !indices || !out) return NJF_E_NULL;
  const int blocks = (int)(((long long)capacity + 255) / 256);
  field_scatter_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(values, indices, count, capacity, out, out_size);
  return launch_status();
}

extern "C" int njf_field_band_leaks(const NjfFieldGrid* grid, int batch, const unsigned char* band, const int* indices,
                                    const int* count, int capacity, int* leaks, void* stream) {
  FieldList l;
  int rc = make_field_list(grid, batch, nullptr, nullptr, 0, l);
  if (rc) return rc;
  if (capacity < 0) return NJF_E_SHAPE;
  if (!band || !leaks || (capacity > 0 && !indices)) return NJF_E_NULL;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(leaks, 0, sizeof(int), s) != hipSuccess) return launch_status();
  if (capacity == 0) return NJF_OK;
  BandLeakArgs a;
  for (int c = 0; c < 3; ++c) a.dims[c] = grid->dims[c];
  a.nodes = l.nodes;
  a.total = l.total;
  a.band = band;
  a.indices = indices;
  a.count = count;
  a.capacity = capacity;
  a.leaks = leaks;
  const int blocks = (int)(((long long)capacity + NJF_FIELD_BAND_BLOCK - 1) / NJF_FIELD_BAND_BLOCK);
  band_leaks_kernel<<<blocks, NJF_BLOCK_THREADS, 0, s>>>(a);
  return launch_status();
}

extern "C" int njf_field_twists(const float* xyz, const float* jacobian, const int* labels, const float* weights,
                                const int* count, int n, int action_dim, const int* parts, const int* parts_count,
                                int num_parts, int* out_labels, int* out_count, int* nodes, int* status, double* weight,
                                double* centroid, double* omega, double* velocity, double* energy, double* residual,
                                double* q, double* p, double* l, float* row_residual, double* workspace,
                                long long workspace_doubles, int phases, void* stream) {
  if (action_dim < 1 || action_dim > NJF_MAX_ACTION_DIM) return NJF_E_VALUE;
  if (num_parts < 1 || num_parts > NJF_FIELD_TWISTS_MAX_PARTS) return NJF_E_VALUE;
  if (phases < 1 || phases > NJF_FIELD_TWISTS_ALL) return NJF_E_VALUE;
  if (n < 0) return NJF_E_SHAPE;
  const int chunks = (int)(((long long)n + NJF_FIELD_TWISTS_CHUNK - 1) / NJF_FIELD_TWISTS_CHUNK);
  const int stride = NJF_FIELD_TWISTS_STRIDE(action_dim);
  const long long need = (long long)num_parts * chunks * stride;
  if (need > 0x7fffffffLL || workspace_doubles < need) return NJF_E_SHAPE;
  if (!parts || !out_labels || !out_count || !nodes || !status || !weight || !centroid || !omega || !velocity || !energy ||
      !residual || !q || !p || !l)
    return NJF_E_NULL;
  if (n > 0 && (!xyz || !jacobian || !labels || !row_residual || !workspace)) return NJF_E_NULL;
  TwistArgs a{xyz, jacobian, labels, weights, count, n, action_dim, parts, parts_count, num_parts, chunks, stride,
              out_labels, out_count, nodes, status, weight, centroid, omega, velocity, energy, residual, q, p, l,
              row_residual, workspace};
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(chunks, num_parts);
  int rc;
  // (the phases exist to time the launches apart: each reads what the earlier ones left in the outputs and the workspace)
  if (n > 0 && (phases & NJF_FIELD_TWISTS_CLEAR)) {
    if (hipMemsetAsync(row_residual, 0, (size_t)n * sizeof(float), s) != hipSuccess) return launch_status();
  }
  if (n > 0 && (phases & NJF_FIELD_TWISTS_SUMS)) {
    twist_sums_kernel<<<grid, NJF_TWIST_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  if (phases & NJF_FIELD_TWISTS_CENTROID) {
    twist_centroid_kernel<<<num_parts, 64, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  if (n > 0 && (phases & NJF_FIELD_TWISTS_MOMENTS)) {
    twist_moments_kernel<<<grid, NJF_TWIST_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  if (phases & NJF_FIELD_TWISTS_SOLVE) {
    twist_solve_kernel<<<num_parts, 128, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  if (n > 0 && (phases & NJF_FIELD_TWISTS_RESIDUAL)) {
    twist_residual_kernel<<<grid, NJF_TWIST_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  if (phases & NJF_FIELD_TWISTS_RESIDUAL_SUM) {
    twist_residual_sum_kernel<<<num_parts, 64, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  return NJF_OK;
}

extern "C" int njf_field_joints(const NjfFieldGrid* grid, int batch, const int* indices, const int* labels, const int* count,
                                int n, const int* parts, const int* parts_count, int num_parts, const int* part_status,
                                const double* centroid, const double* omega, const double* velocity, int action_dim,
                                int connectivity, int min_contacts, int max_joints, int* part_a, int* part_b,
                                long long* contacts, int* status, int* out_count, double* anchor, double* out_omega,
                                double* out_velocity, long long* workspace, long long workspace_words, int phases,
                                void* stream) {
  if (connectivity != 6 && connectivity != 14) return NJF_E_VALUE;
  if (num_parts < 1 || num_parts > NJF_FIELD_TWISTS_MAX_PARTS) return NJF_E_VALUE;
  if (action_dim < 1 || action_dim > NJF_MAX_ACTION_DIM) return NJF_E_VALUE;
  if (max_joints < 1 || max_joints > NJF_FIELD_JOINTS_MAX) return NJF_E_VALUE;
  if (min_contacts < 1) return NJF_E_VALUE;
  if (phases < 1 || phases > (NJF_FIELD_JOINTS_ALL | NJF_FIELD_JOINTS_PER_LANE)) return NJF_E_VALUE;
  if (n < 0) return NJF_E_SHAPE;
  FieldList l;
  int rc = make_field_list(grid, batch, nullptr, nullptr, 0, l);  // B*N < 2^31
  if (rc) return rc;
  // the table [K][K][4] of 64-bit words first, the volume [B*N] of 32-bit words behind it
  const long long table_words = NJF_FIELD_JOINTS_TABLE_WORDS(num_parts);
  if (workspace_words < NJF_FIELD_JOINTS_WORKSPACE(l.total, num_parts)) return NJF_E_SHAPE;
  if (!parts || !part_status || !centroid || !omega || !velocity || !part_a || !part_b || !contacts || !status || !out_count ||
      !anchor || !out_omega || !out_velocity || !workspace)
    return NJF_E_NULL;
  if (n > 0 && (!indices || !labels)) return NJF_E_NULL;
  JointArgs a;
  for (int c = 0; c < 3; ++c) {
    a.dims[c] = grid->dims[c];
    a.origin[c] = grid->origin[c];
    a.step[c] = grid->step[c];
  }
  a.nodes = l.nodes;
  a.total = l.total;
  a.indices = indices;
  a.labels = labels;
  a.count = count;
  a.n = n;
  a.parts = parts;
  a.parts_count = parts_count;
  a.K = num_parts;
  a.A = action_dim;
  a.half = connectivity / 2;
  a.min_contacts = min_contacts;
  a.J = max_joints;
  a.part_status = part_status;
  a.centroid = centroid;
  a.omega = omega;
  a.velocity = velocity;
  a.table = (unsigned long long*)workspace;
  a.volume = (int*)(workspace + table_words);
  a.part_a = part_a;
  a.part_b = part_b;
  a.status = status;
  a.out_count = out_count;
  a.contacts = contacts;
  a.anchor = anchor;
  a.out_omega = out_omega;
  a.out_velocity = out_velocity;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = (int)(((long long)n + NJF_JOINT_THREADS - 1) / NJF_JOINT_THREADS);
  // (the phases exist to time the launches apart: each reads what the earlier ones left in the workspace and the outputs)
  if (phases & NJF_FIELD_JOINTS_CLEAR) {
    if (hipMemsetAsync(a.volume, 0xff, (size_t)l.total * sizeof(int), s) != hipSuccess) return launch_status();
    if (hipMemsetAsync(a.table, 0, (size_t)table_words * sizeof(long long), s) != hipSuccess) return launch_status();
  }
  if (n > 0 && (phases & NJF_FIELD_JOINTS_SLOTS)) {
    joint_slots_kernel<<<blocks, NJF_JOINT_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  if (n > 0 && (phases & NJF_FIELD_JOINTS_CONTACTS)) {
    if (phases & NJF_FIELD_JOINTS_PER_LANE) joint_contacts_kernel<false><<<blocks, NJF_JOINT_THREADS, 0, s>>>(a);
    else joint_contacts_kernel<true><<<blocks, NJF_JOINT_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  if (phases & NJF_FIELD_JOINTS_LIST) {
    joint_list_kernel<<<1, NJF_JOINT_LIST_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  if (phases & NJF_FIELD_JOINTS_TWISTS) {
    joint_twists_kernel<<<(max_joints * action_dim + NJF_JOINT_THREADS - 1) / NJF_JOINT_THREADS, NJF_JOINT_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  return NJF_OK;
}

extern "C" int njf_field_pose(const int* parts, const int* parts_count, int num_parts, const int* part_status,
                              const double* centroid, const double* omega, const double* velocity, int action_dim,
                              const int* part_a, const int* part_b, const int* joints_count, int max_joints,
                              const double* anchor, const double* joint_omega, const double* joint_velocity, const int* parent,
                              const int* joint_of, const float* commands, int num_commands, double* rotation,
                              double* translation, int* status, int* depth, const float* xyz, const int* labels,
                              const int* count, int n, const float* jacobian, float* posed, double* workspace,
                              long long workspace_doubles, int phases, void* stream) {
  if (num_parts < 1 || num_parts > NJF_FIELD_TWISTS_MAX_PARTS) return NJF_E_VALUE;
  if (action_dim < 1 || action_dim > NJF_MAX_ACTION_DIM) return NJF_E_VALUE;
  if (num_commands < 1 || num_commands > NJF_FIELD_POSE_MAX_COMMANDS) return NJF_E_VALUE;
  const bool tree = part_a || part_b || joints_count || anchor || joint_omega || joint_velocity || parent || joint_of;
  if (tree && (max_joints < 1 || max_joints > NJF_FIELD_JOINTS_MAX)) return NJF_E_VALUE;
  if (phases < 1 || phases > (NJF_FIELD_POSE_ALL | NJF_FIELD_POSE_STAGED | NJF_FIELD_POSE_WIDE)) return NJF_E_VALUE;
  if (n < 0) return NJF_E_SHAPE;
  // (the links launch reads the twists, links and chain the workspace; the points launch needs neither)
  const bool links = phases & NJF_FIELD_POSE_LINKS, walk = phases & (NJF_FIELD_POSE_LINKS | NJF_FIELD_POSE_CHAIN);
  if (walk && workspace_doubles < NJF_FIELD_POSE_WORKSPACE(num_commands, num_parts)) return NJF_E_SHAPE;
  if (!parts || !commands || !rotation || !translation || !status || !depth || (walk && !workspace)) return NJF_E_NULL;
  if (links && (!part_status || !centroid || !omega || !velocity)) return NJF_E_NULL;
  // joints and tree come together or not at all (joints_count alone may be absent: NULL = max_joints)
  if (tree && (!part_a || !part_b || !anchor || !joint_omega || !joint_velocity || !parent || !joint_of)) return NJF_E_NULL;
  const bool points = xyz || labels || posed || jacobian || count;
  if (points && n > 0 && (!xyz || !labels || !posed)) return NJF_E_NULL;
  PoseArgs a;
  a.parts = parts;
  a.parts_count = parts_count;
  a.K = num_parts;
  a.A = action_dim;
  a.J = tree ? max_joints : 0;
  a.M = num_commands;
  a.part_status = part_status;
  a.centroid = centroid;
  a.omega = omega;
  a.velocity = velocity;
  a.part_a = part_a;
  a.part_b = part_b;
  a.joints_count = joints_count;
  a.anchor = anchor;
  a.joint_omega = joint_omega;
  a.joint_velocity = joint_velocity;
  a.parent = parent;
  a.joint_of = joint_of;
  a.commands = commands;
  a.link = workspace;
  a.link_bits = (int*)(workspace + 12LL * num_commands * num_parts);
  a.rotation = rotation;
  a.translation = translation;
  a.status = status;
  a.depth = depth;
  a.xyz = xyz;
  a.labels = labels;
  a.count = count;
  a.n = n;
  a.jacobian = jacobian;
  a.posed = posed;
  hipStream_t s = (hipStream_t)stream;
  int rc;
  const int blocks = (num_commands * num_parts + NJF_POSE_THREADS - 1) / NJF_POSE_THREADS;  // M*K <= 65535 * 256
  if (phases & NJF_FIELD_POSE_LINKS) {
    pose_links_kernel<<<blocks, NJF_POSE_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  if (phases & NJF_FIELD_POSE_CHAIN) {
    pose_chain_kernel<<<blocks, NJF_POSE_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  if (points && n > 0 && (phases & NJF_FIELD_POSE_POINTS)) {
    const dim3 grid((unsigned)(((long long)n + NJF_POSE_THREADS - 1) / NJF_POSE_THREADS),
                    (unsigned)((num_commands + NJF_POSE_COMMAND_TILE - 1) / NJF_POSE_COMMAND_TILE));  // y <= 2048
    const bool staged = phases & NJF_FIELD_POSE_STAGED, wide = phases & NJF_FIELD_POSE_WIDE;
    if (staged && wide) pose_points_kernel<true, true><<<grid, NJF_POSE_THREADS, 0, s>>>(a);
    else if (staged) pose_points_kernel<true, false><<<grid, NJF_POSE_THREADS, 0, s>>>(a);
    else if (wide) pose_points_kernel<false, true><<<grid, NJF_POSE_THREADS, 0, s>>>(a);
    else pose_points_kernel<false, false><<<grid, NJF_POSE_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  return NJF_OK;
}

// njf_field_commands and njf_field_commands_metric: the checks and the three launches, `metric` choosing the 74-moment kernels
static int ik_entry(bool metric, const float* information, int information_per_problem, const int* parts, const int* parts_count,
                    int num_parts, const int* part_status, const double* centroid, const double* omega, const double* velocity,
                    int action_dim, const int* part_a, const int* part_b, const int* joints_count, int max_joints,
                    const double* anchor, const double* joint_omega, const double* joint_velocity, const int* parent,
                    const int* joint_of, const float* xyz, const int* labels, const int* count, int n, const float* targets,
                    int num_problems, const float* weights, int weights_per_problem, const float* init, const float* lower,
                    const float* upper, double reg, int iterations, double damping, float* commands, double* cost,
                    double* initial_cost, double* weight, int* steps, double* gradient, int* status, int* out_part_status,
                    int* depth, double* moments, double* workspace, long long workspace_doubles, int phases, void* stream) {
  if (num_parts < 1 || num_parts > NJF_FIELD_TWISTS_MAX_PARTS) return NJF_E_VALUE;
  if (action_dim < 1 || action_dim > NJF_MAX_ACTION_DIM) return NJF_E_VALUE;
  if (num_problems < 1 || num_problems > NJF_FIELD_POSE_MAX_COMMANDS) return NJF_E_VALUE;
  const bool tree = part_a || part_b || joints_count || anchor || joint_omega || joint_velocity || parent || joint_of;
  if (tree && (max_joints < 1 || max_joints > NJF_FIELD_JOINTS_MAX)) return NJF_E_VALUE;
  const bool butterfly = metric && (phases & NJF_FIELD_COMMANDS_METRIC_BUTTERFLY);
  if (butterfly) phases &= ~NJF_FIELD_COMMANDS_METRIC_BUTTERFLY;  // (a modifier of the moments phase)
  if (phases < 1 || phases > NJF_FIELD_COMMANDS_ALL || (butterfly && !(phases & NJF_FIELD_COMMANDS_MOMENTS))) return NJF_E_VALUE;
  if (metric && (information_per_problem < 0 || information_per_problem > 1)) return NJF_E_VALUE;
  if (iterations < 0 || iterations > NJF_FIELD_COMMANDS_MAX_ITERATIONS) return NJF_E_VALUE;
  if (!(damping > 0.0) || !(reg >= 0.0) || weights_per_problem < 0 || weights_per_problem > 1) return NJF_E_VALUE;
  if (n < 0) return NJF_E_SHAPE;
  if (workspace_doubles < (metric ? NJF_FIELD_COMMANDS_METRIC_WORKSPACE(num_problems, num_parts, action_dim, n)
                                  : NJF_FIELD_COMMANDS_WORKSPACE(num_problems, num_parts, action_dim, n)))
    return NJF_E_SHAPE;
  if (!parts || !part_status || !centroid || !omega || !velocity || !moments || !out_part_status || !depth || !workspace)
    return NJF_E_NULL;
  if (tree && (!part_a || !part_b || !anchor || !joint_omega || !joint_velocity || !parent || !joint_of)) return NJF_E_NULL;
  const bool sums = phases & NJF_FIELD_COMMANDS_MOMENTS, solve = phases & NJF_FIELD_COMMANDS_SOLVE;
  if (sums && n > 0 && (!xyz || !labels || !targets || (metric && !information))) return NJF_E_NULL;
  if (solve && (!commands || !cost || !initial_cost || !weight || !steps || !gradient || !status)) return NJF_E_NULL;
  IkArgs a;
  PoseArgs& p = a.pose;
  p.parts = parts;
  p.parts_count = parts_count;
  p.K = num_parts;
  p.A = action_dim;
  p.J = tree ? max_joints : 0;
  p.M = num_problems;
  p.part_status = part_status;
  p.centroid = centroid;
  p.omega = omega;
  p.velocity = velocity;
  p.part_a = part_a;
  p.part_b = part_b;
  p.joints_count = joints_count;
  p.anchor = anchor;
  p.joint_omega = joint_omega;
  p.joint_velocity = joint_velocity;
  p.parent = parent;
  p.joint_of = joint_of;
  p.commands = nullptr;
  p.link = nullptr;
  p.link_bits = nullptr;
  p.rotation = p.translation = nullptr;
  p.status = p.depth = nullptr;
  p.xyz = xyz;
  p.labels = labels;
  p.count = count;
  p.n = n;
  p.jacobian = nullptr;
  p.posed = nullptr;
  a.targets = targets;
  a.weights = weights;
  a.weight_stride = weights_per_problem ? n : 0;
  a.information = information;
  a.information_stride = information_per_problem ? 6LL * n : 0;
  a.init = init;
  a.lower = lower;
  a.upper = upper;
  a.reg = reg;
  a.damping = damping;
  a.iterations = iterations;
  a.chunks = (int)(((long long)n + NJF_FIELD_TWISTS_CHUNK - 1) / NJF_FIELD_TWISTS_CHUNK);
  a.partial = workspace;
  a.link_twist = workspace + (size_t)(metric ? NJF_IKM_MOMENTS : NJF_IK_MOMENTS) * a.chunks * num_problems * num_parts;  // [M][2][K][A][6]
  a.moments = moments;
  a.commands = commands;
  a.cost = cost;
  a.initial_cost = initial_cost;
  a.weight = weight;
  a.gradient = gradient;
  a.steps = steps;
  a.status = status;
  a.part_status = out_part_status;
  a.depth = depth;
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (sums) {
    if (n > 0) {  // chunks <= 2^31 / 4096, K <= 256, tiles <= 4096
      const dim3 grid((unsigned)a.chunks, (unsigned)num_parts, (unsigned)((num_problems + NJF_IK_PROBLEM_TILE - 1) / NJF_IK_PROBLEM_TILE));
      if (!metric) ik_moments_kernel<<<grid, NJF_IK_THREADS, 0, s>>>(a);
      else if (butterfly) ikm_moments_kernel<true><<<grid, NJF_IK_THREADS, 0, s>>>(a);
      else ikm_moments_kernel<false><<<grid, NJF_IK_THREADS, 0, s>>>(a);
      if ((rc = launch_status())) return rc;
    }
    const dim3 grid((unsigned)num_parts, (unsigned)((num_problems + NJF_IK_FINISH_TILE - 1) / NJF_IK_FINISH_TILE));
    if (metric) ik_finish_kernel<NJF_IKM_MOMENTS><<<grid, NJF_IK_THREADS, 0, s>>>(a);
    else ik_finish_kernel<NJF_IK_MOMENTS><<<grid, NJF_IK_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  if (solve) {
    if (metric) ik_solve_kernel<true><<<num_problems, NJF_IK_THREADS, 0, s>>>(a);
    else ik_solve_kernel<false><<<num_problems, NJF_IK_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  return NJF_OK;
}

extern "C" int njf_field_commands(const int* parts, const int* parts_count, int num_parts, const int* part_status,
                                  const double* centroid, const double* omega, const double* velocity, int action_dim,
                                  const int* part_a, const int* part_b, const int* joints_count, int max_joints,
                                  const double* anchor, const double* joint_omega, const double* joint_velocity, const int* parent,
                                  const int* joint_of, const float* xyz, const int* labels, const int* count, int n,
                                  const float* targets, int num_problems, const float* weights, int weights_per_problem,
                                  const float* init, const float* lower, const float* upper, double reg, int iterations,
                                  double damping, float* commands, double* cost, double* initial_cost, double* weight, int* steps,
                                  double* gradient, int* status, int* out_part_status, int* depth, double* moments,
                                  double* workspace, long long workspace_doubles, int phases, void* stream) {
  return ik_entry(false, nullptr, 0, parts, parts_count, num_parts, part_status, centroid, omega, velocity, action_dim, part_a, part_b,
                  joints_count, max_joints, anchor, joint_omega, joint_velocity, parent, joint_of, xyz, labels, count, n, targets,
                  num_problems, weights, weights_per_problem, init, lower, upper, reg, iterations, damping, commands, cost,
                  initial_cost, weight, steps, gradient, status, out_part_status, depth, moments, workspace, workspace_doubles,
                  phases, stream);
}

extern "C" int njf_field_commands_metric(const int* parts, const int* parts_count, int num_parts, const int* part_status,
                                         const double* centroid, const double* omega, const double* velocity, int action_dim,
                                         const int* part_a, const int* part_b, const int* joints_count, int max_joints,
                                         const double* anchor, const double* joint_omega, const double* joint_velocity,
                                         const int* parent, const int* joint_of, const float* xyz, const int* labels,
                                         const int* count, int n, const float* targets, const float* information,
                                         int information_per_problem, int num_problems, const float* weights,
                                         int weights_per_problem, const float* init, const float* lower, const float* upper,
                                         double reg, int iterations, double damping, float* commands, double* cost,
                                         double* initial_cost, double* weight, int* steps, double* gradient, int* status,
                                         int* out_part_status, int* depth, double* moments, double* workspace,
                                         long long workspace_doubles, int phases, void* stream) {
  return ik_entry(true, information, information_per_problem, parts, parts_count, num_parts, part_status, centroid, omega, velocity,
                  action_dim, part_a, part_b, joints_count, max_joints, anchor, joint_omega, joint_velocity, parent, joint_of, xyz,
                  labels, count, n, targets, num_problems, weights, weights_per_problem, init, lower, upper, reg, iterations, damping,
                  commands, cost, initial_cost, weight, steps, gradient, status, out_part_status, depth, moments, workspace,
                  workspace_doubles, phases, stream);
}

// The cell list of njf_field_nearest, njf_field_normals and njf_field_voxels.  The lattice checks, all
// NJF_E_VALUE, and the layout of the workspace: Mo (C + 1) words hold the L + 1 starts, L cursors, then the records on the next
// 16 bytes (the macro's 3 spare words).  The caller checks `points`, the workspace's length and its pointer afterwards, in
// its own order: until then `slots` may be anything, and a null workspace leaves the three pointers null.
static int cell_list_make(const NjfFieldGrid* cells, int num_observed, int points, int* workspace, CellList* out) {
  const float cell = cells->step[0], inv_cell = 1.0f / cell;
  if (!(cell > 0.0f) || cells->step[1] != cell || cells->step[2] != cell || !(inv_cell > 0.0f) || !(cell < INFINITY) ||
      !(inv_cell < INFINITY))
    return NJF_E_VALUE;
  long long C = 1;
  for (int c = 0; c < 3; ++c) {
    if (cells->dims[c] < 1 || cells->dims[c] > NJF_FIELD_NEAREST_MAX_DIM) return NJF_E_VALUE;
    if (!(fabsf(cells->origin[c]) < INFINITY)) return NJF_E_VALUE;
    C *= cells->dims[c];
  }
  const long long L = (long long)num_observed * C;
  if (L >= (1LL << 31)) return NJF_E_VALUE;
  for (int c = 0; c < 3; ++c) out->origin[c] = cells->origin[c], out->dims[c] = cells->dims[c];
  out->cell = cell;
  out->inv_cell = inv_cell;
  out->C = (int)C;
  out->Mo = num_observed;
  out->T = points;
  out->L = L;
  out->slots = (long long)num_observed * points;
  out->start = workspace;
  out->cursor = workspace ? workspace + (long long)num_observed * (C + 1) : nullptr;
  out->records = workspace ? (int4*)(((uintptr_t)(out->cursor + L) + 15) & ~(uintptr_t)15) : nullptr;
  return NJF_OK;
}

// the reach of a walk (max_distance, radius) as a float: positive, finite, within NJF_FIELD_NEAREST_MAX_RINGS rings
static int cell_list_reach(const CellList& list, double distance, float* reach) {
  *reach = (float)distance;
  if (!(distance > 0.0) || !(*reach > 0.0f) || !(*reach < INFINITY)) return NJF_E_VALUE;
  if (ceil((double)*reach / (double)list.cell) + 1.0 > (double)NJF_FIELD_NEAREST_MAX_RINGS) return NJF_E_VALUE;
  return NJF_OK;
}

// start[0 .. L]: the exclusive prefix sums of counts[0 .. L), the total at the end; clears the counts
static int exclusive_scan_1024(int* counts, int* start, long long L, hipStream_t s) {
  const int blocks = (int)((L + NJF_NN_SCAN_BLOCK - 1) / NJF_NN_SCAN_BLOCK);  // <= 2^21
  int rc;
  nn_scan_sums_kernel<<<blocks, NJF_NN_THREADS, 0, s>>>(counts, start, L);
  if ((rc = launch_status())) return rc;
  block_offsets_kernel<NJF_NN_SCAN_BLOCK><<<1, NJF_BLOCK_THREADS, 0, s>>>(start, blocks, start + L);
  if ((rc = launch_status())) return rc;
  nn_scan_cells_kernel<<<blocks, NJF_NN_THREADS, 0, s>>>(counts, start, L);
  return launch_status();
}

// a memset and five launches -- count, the scan, fill: the only writer of start and records, and it clears the cursors first
static int cell_list_build(const CellList& list, const float* observed, const int* observed_count, hipStream_t s) {
  const unsigned per_point = (unsigned)((list.slots + NJF_NN_THREADS - 1) / NJF_NN_THREADS);  // < 2^23
  int rc;
  hipError_t e = hipMemsetAsync(list.cursor, 0, (size_t)list.L * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  nn_points_kernel<false><<<per_point, NJF_NN_THREADS, 0, s>>>(list, observed, observed_count);
  if ((rc = launch_status())) return rc;
  if ((rc = exclusive_scan_1024(list.cursor, list.start, list.L, s))) return rc;
  nn_points_kernel<true><<<per_point, NJF_NN_THREADS, 0, s>>>(list, observed, observed_count);
  return launch_status();
}

extern "C" int njf_field_nearest(const float* observed, const int* observed_count, int num_observed, int points,
                                 const float* queries, const int* count, const int* labels, int num_queries, int n,
                                 int num_problems, const NjfFieldGrid* cells, double max_distance, int* index, float* distance2,
                                 float* matched, int* found, int* workspace, long long workspace_words, int phases,
                                 void* stream) {
  if (num_problems < 1 || num_problems > NJF_FIELD_POSE_MAX_COMMANDS) return NJF_E_VALUE;
  if ((num_observed != 1 && num_observed != num_problems) || (num_queries != 1 && num_queries != num_problems)) return NJF_E_VALUE;
  if (phases < 1 || phases > (NJF_FIELD_NEAREST_ALL | NJF_FIELD_NEAREST_WAVE) || !(phases & NJF_FIELD_NEAREST_ALL) ||
      ((phases & NJF_FIELD_NEAREST_WAVE) && !(phases & NJF_FIELD_NEAREST_QUERY)))
    return NJF_E_VALUE;
  if (!cells) return NJF_E_NULL;
  NnArgs a;
  int rc;
  if ((rc = cell_list_make(cells, num_observed, points, workspace, &a.list))) return rc;
  if ((rc = cell_list_reach(a.list, max_distance, &a.max_distance))) return rc;
  if (n < 0 || points < 1 || a.list.slots >= (1LL << 31)) return NJF_E_SHAPE;
  if (workspace_words < NJF_FIELD_NEAREST_WORKSPACE(num_observed, a.list.C, points)) return NJF_E_SHAPE;
  const bool build = phases & NJF_FIELD_NEAREST_BUILD, query = phases & NJF_FIELD_NEAREST_QUERY;
  if (!workspace || (build && !observed) || (query && (!found || (n > 0 && (!queries || !index || !distance2 || !matched)))))
    return NJF_E_NULL;
  a.rows = RowSet{queries, count, labels, num_queries, n};
  a.max_d2 = a.max_distance * a.max_distance;
  a.index = index;
  a.distance2 = distance2;
  a.matched = (int*)matched;
  a.found = found;
  hipStream_t s = (hipStream_t)stream;
  if (build && (rc = cell_list_build(a.list, observed, observed_count, s))) return rc;
  if (query) {
    hipError_t e = hipMemsetAsync(found, 0, (size_t)num_problems * sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    if (n > 0) {
      if (phases & NJF_FIELD_NEAREST_WAVE) {
        const dim3 grid((unsigned)(((long long)n + NJF_NN_THREADS / 64 - 1) / (NJF_NN_THREADS / 64)), (unsigned)num_problems);
        nn_query_kernel<true><<<grid, NJF_NN_THREADS, 0, s>>>(a);
      } else {
        const dim3 grid((unsigned)(((long long)n + NJF_NN_THREADS - 1) / NJF_NN_THREADS), (unsigned)num_problems);
        nn_query_kernel<false><<<grid, NJF_NN_THREADS, 0, s>>>(a);
      }
      if ((rc = launch_status())) return rc;
    }
  }
  return NJF_OK;
}

extern "C" int njf_field_normals(const float* observed, const int* observed_count, int num_observed, int points,
                                 const float* queries, const int* count, int num_queries, int n, int num_problems,
                                 const NjfFieldGrid* cells, double radius, int min_neighbours, const float* viewpoint,
                                 int num_viewpoints, long long* moments, float* normal, int* neighbours, float* variation,
                                 double* eigenvalues, int* workspace, long long workspace_words, int phases, void* stream) {
  if (num_problems < 1 || num_problems > NJF_FIELD_POSE_MAX_COMMANDS) return NJF_E_VALUE;
  if ((num_observed != 1 && num_observed != num_problems) || (num_queries != 1 && num_queries != num_problems)) return NJF_E_VALUE;
  if (viewpoint && num_viewpoints != 1 && num_viewpoints != num_problems) return NJF_E_VALUE;
  if (phases < 1 || phases > (NJF_FIELD_NORMALS_ALL | NJF_FIELD_NORMALS_WAVE) || !(phases & NJF_FIELD_NORMALS_ALL) ||
      ((phases & NJF_FIELD_NORMALS_WAVE) && !(phases & NJF_FIELD_NORMALS_MOMENTS)))
    return NJF_E_VALUE;
  if (min_neighbours < 3) return NJF_E_VALUE;
  if (!cells) return NJF_E_NULL;
  NrmArgs a;
  float reach;
  int rc;
  if ((rc = cell_list_make(cells, num_observed, points, workspace, &a.list))) return rc;
  if ((rc = cell_list_reach(a.list, radius, &reach))) return rc;
  if (n < 0 || points < 1 || points >= (1 << 26) || a.list.slots >= (1LL << 31)) return NJF_E_SHAPE;
  const bool build = phases & NJF_FIELD_NORMALS_BUILD, sums = phases & NJF_FIELD_NORMALS_MOMENTS,
             finish = phases & NJF_FIELD_NORMALS_FINISH;
  if ((build || sums) && workspace_words < NJF_FIELD_NEAREST_WORKSPACE(num_observed, a.list.C, points)) return NJF_E_SHAPE;
  if (((build || sums) && !workspace) || (build && !observed)) return NJF_E_NULL;
  if (n > 0 && (((sums || finish) && (!queries || !moments)) || (finish && (!normal || !neighbours || !variation))))
    return NJF_E_NULL;
  hipStream_t s = (hipStream_t)stream;
  if (build && (rc = cell_list_build(a.list, observed, observed_count, s))) return rc;
  if (n == 0 || !(sums || finish)) return NJF_OK;
  a.rows = RowSet{queries, count, nullptr, num_queries, n};
  a.viewpoint = viewpoint;
  a.Mv = num_viewpoints;
  a.r2 = reach * reach;
  a.rings = 1;  // the smallest r >= 1 whose rings beyond it hold nothing within the radius: nn_query_kernel's second stop test
  while (a.rings < NJF_FIELD_NEAREST_MAX_RINGS && !(((float)a.rings - 0.0078125f) * a.list.cell > reach)) ++a.rings;
  a.scale = 262144.0 / (double)reach;
  a.min_neighbours = min_neighbours;
  a.moments = moments;
  a.normal = normal;
  a.neighbours = neighbours;
  a.variation = variation;
  a.eigenvalues = eigenvalues;
  if (sums) {
    if (phases & NJF_FIELD_NORMALS_WAVE) {
      const dim3 grid((unsigned)(((long long)n + NJF_NN_THREADS / 64 - 1) / (NJF_NN_THREADS / 64)), (unsigned)num_problems);
      nrm_moments_kernel<true><<<grid, NJF_NN_THREADS, 0, s>>>(a);
    } else {
      const dim3 grid((unsigned)(((long long)n + NJF_NN_THREADS - 1) / NJF_NN_THREADS), (unsigned)num_problems);
      nrm_moments_kernel<false><<<grid, NJF_NN_THREADS, 0, s>>>(a);
    }
    if ((rc = launch_status())) return rc;
  }
  if (finish) {
    const dim3 grid((unsigned)(((long long)n + NJF_NN_THREADS - 1) / NJF_NN_THREADS), (unsigned)num_problems);
    nrm_finish_kernel<<<grid, NJF_NN_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  return NJF_OK;
}

extern "C" int njf_field_voxels(const float* points, const int* points_count, int num_problems, int num_points,
                                const NjfFieldGrid* cells, int min_points, int capacity, float* out_points, int* weight,
                                int* cell_index, long long* sums, int* count, int* outside, int* workspace,
                                long long workspace_words, int phases, void* stream) {
  if (num_problems < 1 || num_problems > NJF_FIELD_POSE_MAX_COMMANDS) return NJF_E_VALUE;
  if (phases < 1 || phases > (NJF_FIELD_VOXELS_ALL | NJF_FIELD_VOXELS_WAVE) || !(phases & NJF_FIELD_VOXELS_ALL) ||
      ((phases & NJF_FIELD_VOXELS_WAVE) && !(phases & NJF_FIELD_VOXELS_REDUCE)))
    return NJF_E_VALUE;
  if (min_points < 1) return NJF_E_VALUE;
  if (!cells) return NJF_E_NULL;
  VoxArgs a;
  int rc;
  if ((rc = cell_list_make(cells, num_problems, num_points, workspace, &a.list))) return rc;
  const long long L = a.list.L;
  if (num_points < 1 || a.list.slots >= (1LL << 31)) return NJF_E_SHAPE;
  if (capacity < 1 || (long long)num_problems * capacity >= (1LL << 31)) return NJF_E_SHAPE;
  if (workspace_words < NJF_FIELD_VOXELS_WORKSPACE(num_problems, a.list.C, num_points)) return NJF_E_SHAPE;
  const bool build = phases & NJF_FIELD_VOXELS_BUILD, reduce = phases & NJF_FIELD_VOXELS_REDUCE,
             compact = phases & NJF_FIELD_VOXELS_COMPACT;
  if (!workspace || (build && !points) || (reduce && !outside) ||
      (compact && (!out_points || !weight || !cell_index || !sums || !count)))
    return NJF_E_NULL;
  hipStream_t s = (hipStream_t)stream;
  if (build && (rc = cell_list_build(a.list, points, points_count, s))) return rc;
  a.min_points = min_points;
  a.capacity = capacity;
  a.cell_sums = (long long*)(a.list.records + a.list.slots);  // behind the list: 3 L int64 sums, L counts, L + 1 second starts
  a.cell_k = (int*)(a.cell_sums + 3 * L);
  int* kept_start = a.cell_k + L;
  a.kept_start = kept_start;
  a.points = out_points;
  a.weight = weight;
  a.cell_index = cell_index;
  a.sums = sums;
  a.count = count;
  a.outside = outside;
  if (reduce) {
    hipError_t e = hipMemsetAsync(outside, 0, (size_t)num_problems * sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    if (phases & NJF_FIELD_VOXELS_WAVE)
      vox_reduce_kernel<true><<<(unsigned)((L + NJF_NN_THREADS / 64 - 1) / (NJF_NN_THREADS / 64)), NJF_NN_THREADS, 0, s>>>(a);
    else
      vox_reduce_kernel<false><<<(unsigned)((L + NJF_NN_THREADS - 1) / NJF_NN_THREADS), NJF_NN_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  if (compact) {
    if ((rc = exclusive_scan_1024(a.list.cursor, kept_start, L, s))) return rc;
    const long long threads = L > (long long)num_problems * capacity ? L : (long long)num_problems * capacity;
    vox_scatter_kernel<<<(unsigned)((threads + NJF_NN_THREADS - 1) / NJF_NN_THREADS), NJF_NN_THREADS, 0, s>>>(a);
    if ((rc = launch_status())) return rc;
  }
  return NJF_OK;
}

// ---- which rows a depth camera sees: a z-buffer of points (njf_field_visible) ---------------------------------
// The key image holds (bits(z) << 32) | row per pixel, cleared to all ones; z > near >= 0 is finite, so the bits order as the
// floats do and a 64-bit unsigned minimum picks the smallest z, ties to the lowest row, in any order of arrival.  The splat and the
// test project through the one function below, so a row's own pixel is the same in both.
// The pinhole cameras of njf_field_visible, njf_field_frame and njf_field_tsdf, and the one projection through them.
struct ViewSet {
  const float* k;    // [V,3,3]
  const float* w2c;  // [V,4,4]
  int V, H, W;
  long long pixels;  // H * W
  float near;
};

struct VisArgs {
  RowSet rows;
  ViewSet views;
  int f;
  unsigned chunks;      // workgroups of the resolve per image
  float tolerance;
  unsigned long long* keys;  // [M,V,H,W]
  float* depth;         // [M,V,H,W]
  int* index;           // [M,V,H,W]
  int* covered;         // [M,V]
  int* seen;            // [M,n]
  float* culled;        // [M,n,3]
  int* visible;         // [M]
  int* pixel;           // [M,V,n]
  float* z;             // [M,V,n]
};

struct VisPixel {
  float z, col, row;  // the camera-space z and floor(u W), floor(v H), still floats
  bool projectable;   // z finite and > near
  bool inside;        // projectable and 0 <= col < W, 0 <= row < H
};

// the camera-space z of a world point in the view whose w2c begins at w
__device__ __forceinline__ float camera_z(const float* w, float x, float y, float z) {
  return fmaf(w[10], z, fmaf(w[9], y, fmaf(w[8], x, w[11])));
}

__device__ __forceinline__ VisPixel vis_project(const ViewSet& a, int v, float x, float y, float z) {
  const float* w = a.w2c + v * 16;
  const float* k = a.k + v * 9;
  const float xc = fmaf(w[2], z, fmaf(w[1], y, fmaf(w[0], x, w[3])));
  const float yc = fmaf(w[6], z, fmaf(w[5], y, fmaf(w[4], x, w[7])));
  const float zc = camera_z(w, x, y, z);
  VisPixel p;
  p.z = zc;
  p.projectable = fabsf(zc) < INFINITY && zc > a.near;
  const float s = xc / zc, t = yc / zc;
  const float pu = fmaf(k[1], t, fmaf(k[0], s, k[2]));
  const float pv = fmaf(k[4], t, fmaf(k[3], s, k[5]));
  p.col = floorf(pu * (float)a.W);
  p.row = floorf(pv * (float)a.H);
  p.inside = p.projectable && p.col >= 0.0f && p.col < (float)a.W && p.row >= 0.0f && p.row < (float)a.H;  // (NaN: false)
  return p;
}

// one lane per (m, v, i).  PRE: a plain load of the key first, the atomic only where the key could still fall -- the minimum is
// monotone, so a stale load can only ask for an atomic that changes nothing.
template <bool PRE>
__global__ void __launch_bounds__(256) vis_splat_kernel(VisArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int v = blockIdx.y, m = blockIdx.z;
  const ViewSet& s = a.views;
  if (i >= a.rows.n) return;
  float x, y, z;
  if (!row_read(a.rows, m, i, x, y, z)) return;
  const VisPixel p = vis_project(s, v, x, y, z);
  const float f = (float)a.f;
  // a footprint pixel inside the image: judged in float, before any conversion (NaN and infinities compare false)
  if (!p.projectable || !(p.col >= -f && p.col < (float)s.W + f && p.row >= -f && p.row < (float)s.H + f)) return;
  const int col = (int)p.col, row = (int)p.row;  // |col| <= W + 4, |row| <= H + 4: exact
  const unsigned long long key = ((unsigned long long)__float_as_uint(p.z) << 32) | (unsigned)i;
  unsigned long long* image = a.keys + ((long long)m * s.V + v) * s.pixels;
  const int r0 = max(row - a.f, 0), r1 = min(row + a.f, s.H - 1), c0 = max(col - a.f, 0), c1 = min(col + a.f, s.W - 1);
  for (int r = r0; r <= r1; ++r)
    for (int c = c0; c <= c1; ++c) {
      unsigned long long* slot = image + (long long)r * s.W + c;
      if (PRE && *slot <= key) continue;
      atomicMin(slot, key);
    }
}

// A workgroup covers NJF_VIS_RESOLVE_PIXELS consecutive pixels of ONE image, eight per lane, and adds its winners to the image's
// count with one atomic: the counts of all images lie in one or two cache lines, where the atomics of a wave per 64 pixels
// queued behind each other.
#define NJF_VIS_RESOLVE_PIXELS 2048
__global__ void __launch_bounds__(256) vis_resolve_kernel(VisArgs a) {
  __shared__ int block_won;
  const unsigned image = blockIdx.x / a.chunks;  // < M * V
  const long long first = (long long)(blockIdx.x - image * a.chunks) * NJF_VIS_RESOLVE_PIXELS;
  if (threadIdx.x == 0) block_won = 0;
  __syncthreads();
  int n = 0;
  for (int j = 0; j < NJF_VIS_RESOLVE_PIXELS / 256; ++j) {
    const long long r = first + j * 256 + threadIdx.x;
    bool won = false;
    if (r < a.views.pixels) {
      const long long p = (long long)image * a.views.pixels + r;  // < M * V * H * W
      const unsigned long long key = a.keys[p];
      won = key != ~0ull;
      a.depth[p] = won ? __uint_as_float((unsigned)(key >> 32)) : 0.0f;
      a.index[p] = won ? (int)(unsigned)key : -1;
    }
    n += __popcll(__ballot(won));
  }
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(&block_won, n);
  __syncthreads();
  if (threadIdx.x == 0 && block_won) atomicAdd(&a.covered[image], block_won);
}

// one lane per (m, i)
__global__ void __launch_bounds__(256) vis_test_kernel(VisArgs a) {
  __shared__ int block_seen;
  if (threadIdx.x == 0) block_seen = 0;
  __syncthreads();
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int m = blockIdx.y;
  const ViewSet& s = a.views;
  const bool live = i < a.rows.n;
  unsigned seen = 0;
  if (live) {
    float x = 0.f, y = 0.f, z = 0.f;
    const bool read = row_read(a.rows, m, i, x, y, z);
    for (int v = 0; v < s.V; ++v) {
      int own = -1;
      float zc = __int_as_float(0x7fc00000);
      if (read) {
        const VisPixel p = vis_project(s, v, x, y, z);
        zc = p.z;
        if (p.inside) {
          own = (int)p.row * s.W + (int)p.col;
          const float zmin = a.depth[((long long)m * s.V + v) * s.pixels + own];
          if (__fsub_rn(p.z, zmin) <= __fmul_rn(a.tolerance, zmin)) seen |= 1u << v;
        }
      }
      const long long o = ((long long)m * s.V + v) * a.rows.n + i;
      a.pixel[o] = own;
      a.z[o] = zc;
    }
    const float nan = __int_as_float(0x7fc00000);
    float* c = a.culled + ((long long)m * a.rows.n + i) * 3;
    c[0] = seen ? x : nan;
    c[1] = seen ? y : nan;
    c[2] = seen ? z : nan;
    a.seen[(long long)m * a.rows.n + i] = (int)seen;
  }
  const int n = __popcll(__ballot(seen != 0));  // a workgroup lies in one problem: one atomic for its four waves
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(&block_seen, n);
  __syncthreads();
  if (threadIdx.x == 0 && block_seen) atomicAdd(&a.visible[m], block_seen);
}

// The checks that njf_field_visible, njf_field_frame, njf_field_tsdf and njf_field_tsdf_sample share.  These entries judge in
// classes -- every NJF_E_NULL, then every NJF_E_VALUE, then every NJF_E_SHAPE --, so the problems with their rows and the views
// have one helper per class each; inside a class the order cannot show.
static bool one_or_each(int sets, int num_problems) { return sets == 1 || sets == num_problems; }
static bool nonnegative_finite(float v) { return v >= 0.0f && v < INFINITY; }  // (NaN: false)

// NJF_E_VALUE: M in its range; Mq, Mo, Mf one set for all problems or one each
static int problems_value(int num_problems, int sets_a = 1, int sets_b = 1) {
  if (num_problems < 1 || num_problems > NJF_FIELD_POSE_MAX_COMMANDS) return NJF_E_VALUE;
  return one_or_each(sets_a, num_problems) && one_or_each(sets_b, num_problems) ? NJF_OK : NJF_E_VALUE;
}

// NJF_E_VALUE: V in its range; near and the tolerance finite and not negative
static int views_value(int views, float near, float tolerance = 0.0f) {
  if (views < 1 || views > NJF_FIELD_VISIBLE_MAX_VIEWS) return NJF_E_VALUE;
  return nonnegative_finite(near) && nonnegative_finite(tolerance) ? NJF_OK : NJF_E_VALUE;
}

// NJF_E_SHAPE: n rows with `per_row` outputs each (M, or M V) stay below 2^31
static int rows_shape(int n, long long per_row) { return n < 0 || per_row * n >= (1LL << 31) ? NJF_E_SHAPE : NJF_OK; }

// NJF_E_SHAPE: an image, and the V images of `sets` problems, stay below 2^31 pixels
static int views_shape(long long sets, int views, int height, int width) {
  if (height < 1 || width < 1 || (long long)height * width >= (1LL << 31)) return NJF_E_SHAPE;
  return sets * views * height * width >= (1LL << 31) ? NJF_E_SHAPE : NJF_OK;
}

static ViewSet view_set(const float* k, const float* w2c, int views, int height, int width, float near) {
  return ViewSet{k, w2c, views, height, width, (long long)height * width, near};
}

extern "C" int njf_field_visible(const float* points, const int* count, const int* labels, int num_queries, int n,
                                 int num_problems, const float* k, const float* w2c, int views, int height, int width,
                                 int footprint, float near, float tolerance, float* depth, int* index, int* covered, int* seen,
                                 float* culled, int* visible, int* pixel, float* z, int* workspace, long long workspace_words,
                                 int phases, void* stream) {
  const bool known = phases >= 1 && phases <= (NJF_FIELD_VISIBLE_ALL | NJF_FIELD_VISIBLE_DIRECT) && (phases & NJF_FIELD_VISIBLE_ALL) &&
                     (!(phases & NJF_FIELD_VISIBLE_DIRECT) || (phases & NJF_FIELD_VISIBLE_SPLAT));
  const bool splat = known && (phases & NJF_FIELD_VISIBLE_SPLAT), resolve = known && (phases & NJF_FIELD_VISIBLE_RESOLVE),
             test = known && (phases & NJF_FIELD_VISIBLE_TEST);
  if (!k || !w2c || ((splat || test) && !points) || ((splat || resolve) && !workspace) ||
      ((resolve || test) && !depth) || (resolve && (!index || !covered)) ||
      (test && (!seen || !culled || !visible || !pixel || !z)))
    return NJF_E_NULL;
  if (!known || problems_value(num_problems, num_queries) || views_value(views, near, tolerance)) return NJF_E_VALUE;
  if (footprint < 0 || footprint > NJF_FIELD_VISIBLE_MAX_FOOTPRINT) return NJF_E_VALUE;
  const long long images = (long long)num_problems * views;
  if (views_shape(num_problems, views, height, width) || rows_shape(n, images)) return NJF_E_SHAPE;
  if ((splat || resolve) && workspace_words < NJF_FIELD_VISIBLE_WORKSPACE(num_problems, views, height, width)) return NJF_E_SHAPE;
  VisArgs a;
  a.rows = RowSet{points, count, labels, num_queries, n};
  a.views = view_set(k, w2c, views, height, width, near);
  a.f = footprint;
  const long long pixels = a.views.pixels;
  a.chunks = (unsigned)((pixels + NJF_VIS_RESOLVE_PIXELS - 1) / NJF_VIS_RESOLVE_PIXELS);
  a.tolerance = tolerance;
  a.keys = (unsigned long long*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);  // the spare word of the workspace pays for this
  a.depth = depth;
  a.index = index;
  a.covered = covered;
  a.seen = seen;
  a.culled = culled;
  a.visible = visible;
  a.pixel = pixel;
  a.z = z;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  int rc;
  const unsigned row_blocks = (unsigned)(((long long)n + 255) / 256);
  if (splat) {
    if ((e = hipMemsetAsync(a.keys, 0xff, (size_t)(images * pixels) * sizeof(unsigned long long), s)) != hipSuccess) return (int)e;
    if (n > 0) {
      const dim3 grid(row_blocks, (unsigned)views, (unsigned)num_problems);
      if (phases & NJF_FIELD_VISIBLE_DIRECT)
        vis_splat_kernel<false><<<grid, 256, 0, s>>>(a);
      else
        vis_splat_kernel<true><<<grid, 256, 0, s>>>(a);
      if ((rc = launch_status())) return rc;
    }
  }
  if (resolve) {
    if ((e = hipMemsetAsync(covered, 0, (size_t)images * sizeof(int), s)) != hipSuccess) return (int)e;
    vis_resolve_kernel<<<(unsigned)(images * a.chunks), 256, 0, s>>>(a);  // <= total / 2048 + images < 2^31
    if ((rc = launch_status())) return rc;
  }
  if (test) {
    if ((e = hipMemsetAsync(visible, 0, (size_t)num_problems * sizeof(int), s)) != hipSuccess) return (int)e;
    if (n > 0) {
      vis_test_kernel<<<dim3(row_blocks, (unsigned)num_problems), 256, 0, s>>>(a);
      if ((rc = launch_status())) return rc;
    }
  }
  return NJF_OK;
}

// ---- posed rows against a depth frame by projection (njf_field_frame) --------------------------------------------
// A row is read and projected by row_read and vis_project -- njf_field_visible's own, so pixel and z are its bits --, classified
// against the frame's point at its own pixel, and matched to the closest frame point in the pixel window around it.  The frame is
// njf_field_depth_points' organised cloud: the point of pixel (row, col) of view v is row v*H*W + row*W + col, NaN = none.
struct FrmArgs {
  RowSet rows;
  ViewSet views;
  const float* frame;  // [Mo, V*H*W, 3]
  int Mo, reach;
  bool keep_hidden;
  float tolerance, max_d2;
  int* pixel;          // [M,V,n]
  float* z;            // [M,V,n]
  int* state;          // [M,V,n]
  int* index;          // [M,n]
  float* distance2;    // [M,n]
  int* matched;        // [M,n,3] (the bits of the floats)
  int* found;          // [M]
  int* states;         // [M,5]
};

#define NJF_FRM_THREADS 256
#define NJF_FRM_WAVES (NJF_FRM_THREADS / 64)
static_assert(NJF_FIELD_VISIBLE_MAX_VIEWS < 64, "a row's states are tallied in fields of 6 bits");

// one lane per (m, i): it loops over the views and walks its window.  A workgroup lies in one problem: one atomic per counter
// for its four waves.  (A wave per row, the lanes sharing the window, was built and measured: DESIGN.md section 26.)
__global__ void __launch_bounds__(NJF_FRM_THREADS) frm_match_kernel(FrmArgs a) {
  __shared__ int part[NJF_FIELD_FRAME_STATES + 1][NJF_FRM_WAVES];
  const ViewSet& s = a.views;
  const long long i = (long long)blockIdx.x * NJF_FRM_THREADS + threadIdx.x;
  const int m = blockIdx.y;
  const bool live = i < a.rows.n;
  NnBest b = nn_none();                                    // (j < V H W < 2^31 - 1 beats it at d2 = +inf)
  unsigned tally = 0;                                      // 6 bits per state: the views in which the row has it (<= 32)
  const float* frame = a.frame + (long long)(a.Mo == 1 ? 0 : m) * s.V * s.pixels * 3;
  if (live) {
    float x = 0.f, y = 0.f, z = 0.f;
    const bool read = row_read(a.rows, m, i, x, y, z);
    for (int v = 0; v < s.V; ++v) {
      int own = -1, st = NJF_FIELD_FRAME_OUTSIDE;
      float zc = __int_as_float(0x7fc00000);
      if (read) {
        const VisPixel p = vis_project(s, v, x, y, z);
        zc = p.z;
        if (p.inside) {  // judged in float: 0 <= row < H, 0 <= col < W
          const int row = (int)p.row, col = (int)p.col;
          const int base = (int)(v * s.pixels);  // V H W < 2^31
          own = row * s.W + col;
          const float* f = frame + (long long)(base + own) * 3;
          const float fx = f[0], fy = f[1], fz = f[2];
          if (!nn_finite(fx, fy, fz)) {
            st = NJF_FIELD_FRAME_NO_RETURN;
          } else {
            const float zo = camera_z(s.w2c + v * 16, fx, fy, fz);
            const float slack = __fmul_rn(a.tolerance, zo);
            st = __fsub_rn(zo, zc) > slack ? NJF_FIELD_FRAME_IN_FRONT
                                           : __fsub_rn(zc, zo) > slack ? NJF_FIELD_FRAME_BEHIND : NJF_FIELD_FRAME_ON;
          }
          if (st != NJF_FIELD_FRAME_BEHIND || a.keep_hidden) {
            // the window, clipped to the image before any address is formed: base + r W + c lies in [0, V H W)
            const int r0 = max(row - a.reach, 0), r1 = min(row + a.reach, s.H - 1);
            const int c0 = max(col - a.reach, 0), c1 = min(col + a.reach, s.W - 1);
            for (int r = r0; r <= r1; ++r)
              for (int c = c0; c <= c1; ++c) {
                const int j = base + r * s.W + c;
                const float* q = frame + (long long)j * 3;
                const float px = q[0], py = q[1], pz = q[2];
                if (!nn_finite(px, py, pz)) continue;
                const float dx = x - px, dy = y - py, dz = z - pz;
                nn_take(b, (dx * dx + dy * dy) + dz * dz, j, __float_as_int(px), __float_as_int(py), __float_as_int(pz));
              }
          }
        }
      }
      const long long o = ((long long)m * s.V + v) * a.rows.n + i;
      a.pixel[o] = own;
      a.z[o] = zc;
      a.state[o] = st;
      tally += 1u << (6 * st);
    }
  }
  const bool ok = live && b.j != NJF_NN_NO_INDEX && b.d2 <= a.max_d2;
  if (live) match_store(a.index, a.distance2, a.matched, (long long)m * a.rows.n + i, ok, b);
#pragma unroll
  for (int c = 0; c < NJF_FIELD_FRAME_STATES; ++c) {
    const int t = block_sum((int)((tally >> (6 * c)) & 63u), part[c]);
    if (threadIdx.x == 0 && t) atomicAdd(&a.states[m * NJF_FIELD_FRAME_STATES + c], t);
  }
  const int accepted = block_sum_waves(__popcll(__ballot(ok)), part[NJF_FIELD_FRAME_STATES]);
  if (threadIdx.x == 0 && accepted) atomicAdd(&a.found[m], accepted);
}

extern "C" int njf_field_frame(const float* points, const int* count, const int* labels, int num_queries, int n, int num_problems,
                               const float* frame, int num_frames, const float* k, const float* w2c, int views, int height,
                               int width, int reach, float near, float tolerance, double max_distance, int* pixel, float* z,
                               int* state, int* index, float* distance2, float* matched, int* found, int* states, int phases,
                               void* stream) {
  const bool known = phases == NJF_FIELD_FRAME_MATCH || phases == (NJF_FIELD_FRAME_MATCH | NJF_FIELD_FRAME_KEEP_HIDDEN);
  if (!points || !frame || !k || !w2c || !pixel || !z || !state || !index || !distance2 || !matched || !found || !states)
    return NJF_E_NULL;
  if (!known || problems_value(num_problems, num_queries, num_frames) || views_value(views, near, tolerance)) return NJF_E_VALUE;
  if (reach < 0 || reach > NJF_FIELD_FRAME_MAX_REACH) return NJF_E_VALUE;
  const float limit = (float)max_distance;
  if (!nonnegative_finite(limit)) return NJF_E_VALUE;
  if (views_shape(num_frames, views, height, width) || rows_shape(n, (long long)num_problems * views)) return NJF_E_SHAPE;
  FrmArgs a;
  a.rows = RowSet{points, count, labels, num_queries, n};
  a.views = view_set(k, w2c, views, height, width, near);
  a.frame = frame;
  a.Mo = num_frames;
  a.reach = reach;
  a.keep_hidden = (phases & NJF_FIELD_FRAME_KEEP_HIDDEN) != 0;
  a.tolerance = tolerance;
  a.max_d2 = limit * limit;
  a.pixel = pixel;
  a.z = z;
  a.state = state;
  a.index = index;
  a.distance2 = distance2;
  a.matched = (int*)matched;
  a.found = found;
  a.states = states;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  if ((e = hipMemsetAsync(found, 0, (size_t)num_problems * sizeof(int), s)) != hipSuccess) return (int)e;
  if ((e = hipMemsetAsync(states, 0, (size_t)num_problems * NJF_FIELD_FRAME_STATES * sizeof(int), s)) != hipSuccess) return (int)e;
  if (n > 0) {
    frm_match_kernel<<<dim3((unsigned)(((long long)n + NJF_FRM_THREADS - 1) / NJF_FRM_THREADS), (unsigned)num_problems), NJF_FRM_THREADS, 0,
                       s>>>(a);
    int rc;
    if ((rc = launch_status())) return rc;
  }
  return NJF_OK;
}

// ---- depth frames fused into a truncated signed distance on a grid, and sampled at rows (njf_field_tsdf) --------
// A node is projected by vis_project -- njf_field_visible's own, so its pixel and z are the bits njf_field_visible reports for the
// node as a row --, and a row of the sampler is read by row_read.
struct TsdfArgs {
  ViewSet views;
  NjfFieldGrid grid;
  int nodes;               // N
  const float* depth;      // [M,V,H,W]
  const float* values_in;  // [M,N] or NULL (both or neither)
  const float* weight_in;
  float far, truncation, max_weight;
  float* values;           // [M,N]
  float* weight;           // [M,N]
  int* known;              // [M]
};

#define NJF_TSDF_THREADS 256
#define NJF_TSDF_WAVES (NJF_TSDF_THREADS / 64)

// one lane per (m, g): consecutive lanes are consecutive nodes.  A lane reads and writes its own node only, so the state may be
// the outputs.  A workgroup lies in one problem: one atomic for its four waves.
__global__ void __launch_bounds__(NJF_TSDF_THREADS) tsdf_fuse_kernel(TsdfArgs a) {
  __shared__ int part[NJF_TSDF_WAVES];
  const ViewSet& s = a.views;
  const long long g = (long long)blockIdx.x * NJF_TSDF_THREADS + threadIdx.x;
  const int m = blockIdx.y;
  int has = 0;
  if (g < a.nodes) {
    float x, y, z;
    grid_node(a.grid, (int)g, x, y, z);
    float sum = 0.0f, c = 0.0f;
    for (int v = 0; v < s.V; ++v) {
      const VisPixel p = vis_project(s, v, x, y, z);
      if (!p.inside) continue;  // judged in float: 0 <= row < H, 0 <= col < W
      const float d = a.depth[((long long)m * s.V + v) * s.pixels + ((int)p.row * s.W + (int)p.col)];
      const float sd = __fsub_rn(d, p.z);
      if (fabsf(d) < INFINITY && d > s.near && d <= a.far && sd >= -a.truncation) {  // (NaN: false)
        sum = __fadd_rn(sum, fminf(sd, a.truncation));
        c = __fadd_rn(c, 1.0f);
      }
    }
    const long long o = (long long)m * a.nodes + g;
    const float w0 = a.weight_in ? a.weight_in[o] : 0.0f;
    float value, weight;
    if (c == 0.0f) {
      value = a.values_in ? a.values_in[o] : __int_as_float(0x7fc00000);
      weight = w0;
    } else if (w0 > 0.0f) {
      value = __fdiv_rn(fmaf(w0, a.values_in[o], sum), __fadd_rn(w0, c));
      weight = fminf(__fadd_rn(w0, c), a.max_weight);
    } else {  // nothing fused into the node so far: the old value is not read
      value = __fdiv_rn(sum, c);
      weight = fminf(c, a.max_weight);
    }
    a.values[o] = value;
    a.weight[o] = weight;
    has = weight > 0.0f;
  }
  const int t = block_sum(has, part);
  if (threadIdx.x == 0 && t) atomicAdd(&a.known[m], t);
}

static int check_tsdf_grid(const NjfFieldGrid* grid, int min_dim, long long& nodes) {
  for (int c = 0; c < 3; ++c)
    if (grid->dims[c] < 1) return NJF_E_SHAPE;
  for (int c = 0; c < 3; ++c)
    if (grid->dims[c] < min_dim) return NJF_E_VALUE;
  nodes = (long long)grid->dims[0] * grid->dims[1] * grid->dims[2];
  return nodes >= (1LL << 31) ? NJF_E_SHAPE : NJF_OK;
}

extern "C" int njf_field_tsdf(const NjfFieldGrid* grid, const float* depth, int num_problems, int views, int height, int width,
                              const float* k, const float* w2c, float near, float far, float truncation, float max_weight,
                              const float* values_in, const float* weight_in, float* values, float* weight, int* known,
                              void* stream) {
  if (!grid || !depth || !k || !w2c || !values || !weight || !known || (!values_in != !weight_in)) return NJF_E_NULL;
  if (problems_value(num_problems) || views_value(views, near) || !(far > near)) return NJF_E_VALUE;
  if (!(truncation > 0.0f) || !(truncation < INFINITY) || !(max_weight > 0.0f)) return NJF_E_VALUE;
  long long nodes;
  if (views_shape(num_problems, views, height, width) || check_tsdf_grid(grid, 1, nodes) || num_problems * nodes >= (1LL << 31))
    return NJF_E_SHAPE;  // (with one node per axis allowed, the grid's faults are all of this class)
  TsdfArgs a;
  a.views = view_set(k, w2c, views, height, width, near);
  a.grid = *grid;
  a.nodes = (int)nodes;
  a.depth = depth;
  a.values_in = values_in;
  a.weight_in = weight_in;
  a.far = far;
  a.truncation = truncation;
  a.max_weight = max_weight;
  a.values = values;
  a.weight = weight;
  a.known = known;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  if ((e = hipMemsetAsync(known, 0, (size_t)num_problems * sizeof(int), s)) != hipSuccess) return (int)e;
  tsdf_fuse_kernel<<<dim3((unsigned)((nodes + NJF_TSDF_THREADS - 1) / NJF_TSDF_THREADS), (unsigned)num_problems), NJF_TSDF_THREADS, 0,
                     s>>>(a);
  return launch_status();
}

struct TsdfSampleArgs {
  RowSet rows;
  NjfFieldGrid grid;
  int Mf, nodes;
  const float* values;  // [Mf,N]
  const float* weight;  // [Mf,N]
  int* state;           // [M,n]
  float* distance;      // [M,n]
  float* gradient;      // [M,n,3]
  int* states;          // [M,3]
};

__device__ __forceinline__ float tsdf_lerp(float u, float w, float f) { return fmaf(f, __fsub_rn(w, u), u); }

// one lane per (m, i).  A workgroup lies in one problem: one atomic per counter for its four waves.
__global__ void __launch_bounds__(NJF_TSDF_THREADS) tsdf_sample_kernel(TsdfSampleArgs a) {
  __shared__ int part[NJF_FIELD_TSDF_STATES][NJF_TSDF_WAVES];
  const RowSet& s = a.rows;
  const long long i = (long long)blockIdx.x * NJF_TSDF_THREADS + threadIdx.x;
  const int m = blockIdx.y;
  const bool live = i < s.n;
  int st = NJF_FIELD_TSDF_OUTSIDE;
  if (live) {
    const float nan = __int_as_float(0x7fc00000);
    float distance = nan, gx = nan, gy = nan, gz = nan;
    float x[3] = {0.f, 0.f, 0.f};
    bool in = row_read(s, m, i, x[0], x[1], x[2]);
    int cell[3];
    float f[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float gc = __fdiv_rn(__fsub_rn(x[c], a.grid.origin[c]), a.grid.step[c]);
      in = in && gc >= 0.0f && gc <= (float)(a.grid.dims[c] - 1);  // (NaN: false)
      cell[c] = in ? min((int)floorf(gc), a.grid.dims[c] - 2) : 0;   // 0 <= gc <= dims - 1 < 2^31: the conversion is exact
      f[c] = __fsub_rn(gc, (float)cell[c]);
    }
    if (in) {
      // the cell's eight corners: node (cell + (a, b, c)), every index in [0, N)
      const int nz = a.grid.dims[2], yz = a.grid.dims[1] * nz;
      const long long base = (long long)(a.Mf == 1 ? 0 : m) * a.nodes + ((cell[0] * a.grid.dims[1] + cell[1]) * nz + cell[2]);
      const float* val = a.values + base;
      const float* wgt = a.weight + base;
      float C[2][2][2];
      bool known = true;
#pragma unroll
      for (int ia = 0; ia < 2; ++ia)
#pragma unroll
        for (int ib = 0; ib < 2; ++ib)
#pragma unroll
          for (int ic = 0; ic < 2; ++ic) {
            const int o = ia * yz + ib * nz + ic;
            known = known && !(wgt[o] == 0.0f);
            C[ia][ib][ic] = val[o];
          }
      st = known ? NJF_FIELD_TSDF_KNOWN : NJF_FIELD_TSDF_UNKNOWN;
      if (known) {
        float e[2][2], h[2], q[2], t[2];
#pragma unroll
        for (int ia = 0; ia < 2; ++ia) {
          e[ia][0] = tsdf_lerp(C[ia][0][0], C[ia][0][1], f[2]);
          e[ia][1] = tsdf_lerp(C[ia][1][0], C[ia][1][1], f[2]);
          h[ia] = tsdf_lerp(e[ia][0], e[ia][1], f[1]);
          q[ia] = __fsub_rn(e[ia][1], e[ia][0]);
          t[ia] = tsdf_lerp(__fsub_rn(C[ia][0][1], C[ia][0][0]), __fsub_rn(C[ia][1][1], C[ia][1][0]), f[1]);
        }
        distance = tsdf_lerp(h[0], h[1], f[0]);
        gx = __fdiv_rn(__fsub_rn(h[1], h[0]), a.grid.step[0]);
        gy = __fdiv_rn(tsdf_lerp(q[0], q[1], f[0]), a.grid.step[1]);
        gz = __fdiv_rn(tsdf_lerp(t[0], t[1], f[0]), a.grid.step[2]);
      }
    }
    const long long row = (long long)m * s.n + i;
    a.state[row] = st;
    a.distance[row] = distance;
    a.gradient[row * 3] = gx;
    a.gradient[row * 3 + 1] = gy;
    a.gradient[row * 3 + 2] = gz;
  }
#pragma unroll
  for (int c = 0; c < NJF_FIELD_TSDF_STATES; ++c) {
    const int t = block_sum((int)(live && st == c), part[c]);
    if (threadIdx.x == 0 && t) atomicAdd(&a.states[m * NJF_FIELD_TSDF_STATES + c], t);
  }
}

extern "C" int njf_field_tsdf_sample(const float* points, const int* count, const int* labels, int num_queries, int n,
                                     int num_problems, const NjfFieldGrid* grid, const float* values, const float* weight,
                                     int num_fields, int* state, float* distance, float* gradient, int* states, void* stream) {
  if (!points || !grid || !values || !weight || !state || !distance || !gradient || !states) return NJF_E_NULL;
  if (problems_value(num_problems, num_queries, num_fields)) return NJF_E_VALUE;
  for (int c = 0; c < 3; ++c)
    if (!(grid->step[c] > 0.0f) || !(grid->step[c] < INFINITY) || !(fabsf(grid->origin[c]) < INFINITY)) return NJF_E_VALUE;
  long long nodes;
  int rc;
  if ((rc = check_tsdf_grid(grid, 2, nodes))) return rc;
  if (rows_shape(n, num_problems) || num_fields * nodes >= (1LL << 31)) return NJF_E_SHAPE;
  TsdfSampleArgs a;
  a.rows = RowSet{points, count, labels, num_queries, n};
  a.grid = *grid;
  a.Mf = num_fields;
  a.nodes = (int)nodes;
  a.values = values;
  a.weight = weight;
  a.state = state;
  a.distance = distance;
  a.gradient = gradient;
  a.states = states;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  if ((e = hipMemsetAsync(states, 0, (size_t)num_problems * NJF_FIELD_TSDF_STATES * sizeof(int), s)) != hipSuccess) return (int)e;
  if (n > 0) {
    tsdf_sample_kernel<<<dim3((unsigned)(((long long)n + NJF_TSDF_THREADS - 1) / NJF_TSDF_THREADS), (unsigned)num_problems),
                         NJF_TSDF_THREADS, 0, s>>>(a);
    return launch_status();
  }
  return NJF_OK;
}

extern "C" int njf_resnetfc_backward(const float* d_out, int d_out_dim, const float* activations, const float* w_backward,
                                     int points, float* deltas, float* colsum_partial, const unsigned* masks, int precision,
                                     const float* d_out_absmax, void* deltas16, void* stream) {
  if (!d_out || (!activations && !masks) || !w_backward || !deltas) return NJF_E_NULL;
  if (deltas16 && (!masks || !d_out_absmax)) return NJF_E_NULL;   // the 16-bit storage form reads masks and needs the scale
  if (points < 1 || (long long)points * 11 * 128 > 0x7fffffffffLL) return NJF_E_SHAPE;
  if (d_out_dim < 1 || d_out_dim > 32) return NJF_E_DOUT;
  BackwardArgs a{d_out, d_out_dim, activations, w_backward, points, deltas, colsum_partial, masks, d_out_absmax, (_Float16*)deltas16};
  if (precision == NJF_PRECISION_F16X2) {
    if (!d_out_absmax) return NJF_E_NULL;
    return launch_fused(resnetfc_backward_kernel<PREC_F16X2>, a, (points + 31) / 32, (hipStream_t)stream);
  }
  if (precision != NJF_PRECISION_F32) return NJF_E_MODE;
  return launch_fused(resnetfc_backward_kernel<PREC_F32>, a, (points + 31) / 32, (hipStream_t)stream);
}

extern "C" int njf_pack_transformer_backward(const float* mats, const float* biases, const float* head_w, int d_out,
                                             float* w_out, float* b_out, int precision, void* stream) {
  // mats [3][4][64][64] row-major [out][in] = (Mqk, Nov, W1', W2) per layer; biases [3][3][64] = (bqk, bo, b1') per layer;
  // head_w [d_out][64] = the output Linear.  w_out: NJF_TRANSFORMER_BACKWARD_CHUNKS chunks, b_out [3][192]
  if (!mats || !biases || !head_w || !w_out || !b_out) return NJF_E_NULL;
  if (d_out < 1 || d_out > 32) return NJF_E_DOUT;
  if (precision != NJF_PRECISION_F32 && precision != NJF_PRECISION_F16X2) return NJF_E_MODE;
  hipStream_t s = (hipStream_t)stream;
  const int P = precision;
  fill_kernel<<<64, 256, 0, s>>>(w_out, NJF_TRANSFORMER_BACKWARD_CHUNKS * NJF_CHUNK_FLOATS, 0.f);
  PackScope scope(s);   // 22 matrices: one launch, after the fill
  launch_pack(head_w, nullptr, 64, d_out, 2, 1, 3, P, w_out, nullptr, s);                      // Wj^T: 64 rows, K = d_out (<= 32)
  for (int l = 2, c = 1; l >= 0; --l, c += 4) {
    const float* m = mats + (size_t)l * 4 * 4096;
    const float* b = biases + (size_t)l * 192;
    float* base = w_out + (size_t)c * NJF_CHUNK_FLOATS;
    launch_pack(m, b, 64, 64, 2, 2, 0, P, base, b_out + 192 * l, s);                           // Mqk (+ bqk)
    launch_pack(m + 4096, b + 64, 64, 64, 2, 2, 0, P, base + 4096, b_out + 192 * l + 64, s);   // Nov (+ bo)
    launch_pack(m + 2 * 4096, b + 128, 64, 64, 2, 2, 0, P, base + NJF_CHUNK_FLOATS, b_out + 192 * l + 128, s);   // W1' (+ b1')
    launch_pack(m + 3 * 4096, nullptr, 64, 64, 2, 2, 3, P, base + NJF_CHUNK_FLOATS + 4096, nullptr, s);          // W2^T
    launch_pack(m + 2 * 4096, nullptr, 64, 64, 2, 2, 3, P, base + 2 * NJF_CHUNK_FLOATS, nullptr, s);             // W1'^T
    launch_pack(m + 4096, nullptr, 64, 64, 2, 2, 3, P, base + 2 * NJF_CHUNK_FLOATS + 4096, nullptr, s);          // Nov^T
    launch_pack(m, nullptr, 64, 64, 2, 2, 3, P, base + 3 * NJF_CHUNK_FLOATS, nullptr, s);                        // Mqk^T
  }
  scope.flush();   // (before the status query: a failed batch launch must be this call's error)
  return launch_status();
}

extern "C" int njf_transformer_backward(const float* x, const float* d_out, int d_out_dim, int keys, int points,
                                        const float* w_backward, const float* b_backward, float* wg_x, float* wg_dy,
                                        float* dx0, float* colsum_partial, int half_storage, const float* d_out_absmax,
                                        int precision, void* stream) {
  if (!x || !d_out || !w_backward || !b_backward || !wg_x || !wg_dy || !dx0) return NJF_E_NULL;
  if (points < 1 || (long long)points * 12 * 64 > 0x7fffffffffLL) return NJF_E_SHAPE;
  if (d_out_dim < 1 || d_out_dim > 32) return NJF_E_DOUT;
  if (keys < 1 || keys > 8) return NJF_E_ACTION_DIM;
  if (half_storage && !d_out_absmax) return NJF_E_NULL;
  TransformerBwdArgs a{x, d_out, d_out_dim, keys, points, w_backward, b_backward, wg_x, wg_dy, dx0, colsum_partial,
                       half_storage != 0, d_out_absmax};
  if (precision == NJF_PRECISION_F16X2) {
    if (!d_out_absmax) return NJF_E_NULL;
    return launch_fused(transformer_backward_kernel<PREC_F16X2>, a, (points + 31) / 32, (hipStream_t)stream);
  }
  if (precision != NJF_PRECISION_F32) return NJF_E_MODE;
  return launch_fused(transformer_backward_kernel<PREC_F32>, a, (points + 31) / 32, (hipStream_t)stream);
}

