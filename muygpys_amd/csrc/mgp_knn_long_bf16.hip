// Exact k-nearest-neighbour scan for rows of 68 to 256 features with a split-bf16 pre-filter (k <= 64).
//
// The contract of knn_scan_bf16x3_kernel (csrc/mgp_knn.hip) on the rows of csrc/mgp_knn_long.hip: every fp32 feature is
// split x = hi + lo + r on the host (rows packed [hi(KP) | lo(KP)] in bf16, KP = 16 ceil((d + 2) / 16) = 80 .. 272), three
// v_mfma_f32_32x32x16_bf16 chains hi.hi + hi.lo + lo.hi give q.x, and the last two packed slots carry (c, 1) in a table
// row and (1, -thr) in a query row, so the accumulator IS q.x + c - thr: a pair survives iff it is positive, and per
// 32 x 32 block the vector unit only takes the max over a lane's 16 accumulators.  Survivors go into 16-entry per-query
// queues and are re-measured EXACTLY (fp32 difference form, from the fp32 tables) when the queue drains: the lists and tau
// only ever hold exact distances.  overflow[q] = 1 where a queue overflowed.
//
// That kernel keeps whole packed rows of both operands resident or staged (and spills at KP = 48).  This one is chunked:
//
//   A operand   the wave's queries, whole packed rows, in registers for the whole scan.  Packed slots are taken in
//               16-byte PIECES of eight: matrix step J (K = 16) multiplies pieces 2 J (lanes 0-31) and 2 J + 1 (lanes
//               32-63), so lane (r32, half) holds pieces 2 J + half, J < NQ = KP / 16, of the hi and of the lo part:
//               8 NQ registers per 32-query row block (136 at KP = 272).  Two row blocks per wave up to NQ = 6 (d <= 92),
//               one beyond.  The -thr slot (KP - 1) is the upper half-word of the last register of piece NQ - 1 of the
//               upper lanes; when a query's tau tightens that lane rewrites it in place (neg_thr_split_long).
//   table side  a 64-row tile is staged in NCH = ceil(NQ / 4) chunks of NQ / NCH (+ 1) steps -- never more than the NQ
//               steps the row has, no rounding up to 4 NCH -- each chunk the hi pieces AND the lo pieces of one step range,
//               so the three chains of a chunk run from one buffer.  Row stride 4 S + 1 sixteen-byte slots for a chunk of
//               S steps (odd: 32 consecutive rows read conflict-free), filled by global_load_lds, double-buffered over
//               the (tile, chunk) sequence with one barrier per chunk.  The two x RBN 32 x 32 accumulators of a wave
//               carry across the chunks of a tile; the last chunk holds the two threshold slots.  2 x 17 KB of tile
//               whatever d is (a whole packed tile at KP = 272 would be 68 KB).
//   drain       the cadence and the walk order of knn_scan_long_kernel (every tile up to 64, then every 4 / 8 / 16;
//               workgroup b starts at tile 7919 b mod ntiles); the queue, the lane-per-query exact re-measurement and
//               the list insertion of knn_scan_bf16x3_kernel.
//
// The margin.  Per element |lo| <= 2^-8 |x| and |r| <= 2^-16 |x|, so the dropped terms lo.lo + r.x + q.r are at most
// 3.1 x 2^-16 sum |q_i x_i|.  One accumulator sums N = 3 KP products, each exact in fp32 (8 x 8 significand bits); the
// matrix unit's order and rounding of the additions are not specified, so each is allowed a unit roundoff of 2^-23:
// |error| <= g_N sum |t_i|, g_N = N 2^-23 / (1 - N 2^-23), over ALL N terms.  The feature terms: sum |t_i| <=
// (1 + 2^-7) sum |q_i x_i| <= 1.01 |q| |x| (Cauchy-Schwarz), so
//         |computed q.x - q.x| <= E(KP) |q| |x|,   E(KP) = 3.1 x 2^-16 + 1.01 x 3 KP x 2^-23
// (KP = 80: 5.0 x 2^-16; KP = 272: 9.6 x 2^-16 = 2.4 x 2^-14 -- the 2^-14 of the short rows, derived for 240 products,
// does not cover it).  The host folds E(KP) QMAX |x| into c.  The two threshold terms take part in the same sum: c is
// raised by R(KP) |c| and thr lowered by R(KP) |thr| + 2^-23 |q|^2, R(KP) = 2^-16 + 1.01 x 3 KP x 2^-23: g_N of the
// term itself, the split's own error (2^-18) and the rounding of |x|^2, |q|^2 to fp32.  (neighbors.py: prefilter_margin,
// prefilter_raise.)
//
// Resources (lib/kernel_resources.json; tests/test_knn_long_bf16_status_cpu.py compares this table with the report).
// NQ = KP / 16, RBN row blocks per wave, 128 RBN queries per workgroup of four waves:
//
//   kernel                        NQ  RBN  VGPRs  AGPRs  waves/SIMD  VGPR spill  scratch
//   knn_prefilter_long_kernel      5    2    240      0       2           0         0
//   knn_prefilter_long_kernel      6    2    254      0       2           0         0
//   knn_prefilter_long_kernel      7    1    162      0       3           0         0
//   knn_prefilter_long_kernel      8    1    168      0       3           0         0
//   knn_prefilter_long_kernel      9    1    182      0       2           0         0
//   knn_prefilter_long_kernel     10    1    190      0       2           0         0
//   knn_prefilter_long_kernel     11    1    202      0       2           0         0
//   knn_prefilter_long_kernel     12    1    210      0       2           0         0
//   knn_prefilter_long_kernel     13    1    214      0       2           0         0
//   knn_prefilter_long_kernel     14    1    228      0       2           0         0
//   knn_prefilter_long_kernel     15    1    236      0       2           0         0
//   knn_prefilter_long_kernel     16    1    240      0       2           0         0
//   knn_prefilter_long_kernel     17    1    256      0       2           0         0
//
// (Seven steps with two row blocks spill 15 registers at the 256 of two waves per SIMD: one row block from there on.)
// Dynamic LDS: 2 x 17 KB of tile + 128 RBN x (16 queue entries + counter + tau) = 43 KB (RBN = 1) / 52 KB (RBN = 2):
// two workgroups per CU either way.
#include <cstdint>
#include <type_traits>
#include <utility>

#include "mgp_args.h"
#include "mgp_knn_common.h"

namespace mgp {
namespace {

constexpr int PL_SC = 4;                                  // matrix steps per chunk, at most
constexpr int PL_BUF = KNN_TN * (4 * PL_SC + 1) * 16;     // bytes of one staging buffer: 64 rows x 17 slots
constexpr int PL_RB2_MAX_NQ = 6;                          // two row blocks per wave up to this many steps (the register report)
constexpr int PL_SCAN_BLOCK = 16;                         // list entries loaded together when a survivor is inserted

constexpr int pl_nch(int nq) { return (nq + PL_SC - 1) / PL_SC; }
constexpr int pl_steps(int nq, int c) { return nq / pl_nch(nq) + (c < nq % pl_nch(nq) ? 1 : 0); }
constexpr int pl_first(int nq, int c) { return c * (nq / pl_nch(nq)) + (c < nq % pl_nch(nq) ? c : nq % pl_nch(nq)); }
constexpr int pl_rbn(int nq) { return nq <= PL_RB2_MAX_NQ ? 2 : 1; }
constexpr size_t pl_lds_bytes(int rbn) { return 2 * PL_BUF + (size_t)KNN_QB * rbn * (KNN_CAP + 2) * sizeof(int); }

template <typename F, int... I>
__device__ __forceinline__ void pl_static_for(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}

__device__ __forceinline__ unsigned pl_bf16_rne(float x) {  // bits of bf16(x), round to nearest even
  const unsigned u = __float_as_uint(x);
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
// -thr as (hi, lo) bf16 bits, thr = (|q|^2 - tau) / 2 first lowered by R(KP) |thr| + 2^-23 |q|^2 (the header comment)
template <int NQ>
__device__ __forceinline__ void neg_thr_split_long(float qn, float tau, unsigned& hi, unsigned& lo) {
  constexpr float R = 0x1p-16f + 1.01f * (48 * NQ) * 0x1p-23f;
  float thr = fminf(0.5f * (qn - tau), 1e38f);  // tau = -inf (rows past the end): nothing ever passes
  thr -= R * fabsf(thr) + 0x1p-23f * qn;
  const float v = -thr;
  hi = pl_bf16_rne(v);
  lo = pl_bf16_rne(v - __uint_as_float(hi << 16));
}

}  // namespace

template <int NQ, int RBN>
__global__ __launch_bounds__(256, 2) void knn_prefilter_long_kernel(KnnPackedArgs a) {
  constexpr int KP = 16 * NQ;
  constexpr int RB = 4 * KP;            // bytes of a packed row
  constexpr int NCH = pl_nch(NQ);
  constexpr int QW = KNN_QW * RBN;      // queries per wave
  constexpr int QB = KNN_QB * RBN;      // queries per workgroup
  extern __shared__ __attribute__((aligned(16))) char smem[];  // carved by hand
  char* tile0 = smem;                                              // [2][PL_BUF]
  int* q_i = reinterpret_cast<int*>(smem + 2 * PL_BUF);            // [QB * KNN_CAP]
  int* q_cnt = q_i + QB * KNN_CAP;                                 // [QB]
  float* tau_s = reinterpret_cast<float*>(q_cnt + QB);             // [QB]

  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int half = lane >> 5, r32 = lane & 31;
  const int64_t qbase = (int64_t)blockIdx.x * QB;
  const int d = a.d, k = a.k;
  const char* ptrain = reinterpret_cast<const char*>(a.packed_train);

  for (int t = tid; t < QB; t += 256) {
    const int64_t q = qbase + t;
    float tau = -__builtin_inff();  // rows past the end never accept anything
    if (q < a.m) {
      tau = a.best_d[q * k];
      for (int j = 1; j < k; ++j) tau = fmaxf(tau, a.best_d[q * k + j]);
    }
    tau_s[t] = tau;
    q_cnt[t] = 0;
  }
  __syncthreads();
  // A operands: row block rb, lane (r32, half): pieces 2 J + half of query qbase + QW w + 32 rb + r32, hi and lo parts
  u4x ahi[RBN][NQ], alo[RBN][NQ];
  float myqn[RBN];
  auto set_thr = [&](int rb, float tau) {  // (upper lanes) -thr of the row block's query into packed slot KP - 1
    unsigned hi, lo;
    neg_thr_split_long<NQ>(myqn[rb], tau, hi, lo);
    ahi[rb][NQ - 1].w = (ahi[rb][NQ - 1].w & 0xFFFFu) | (hi << 16);
    alo[rb][NQ - 1].w = (alo[rb][NQ - 1].w & 0xFFFFu) | (lo << 16);
  };
#pragma unroll
  for (int rb = 0; rb < RBN; ++rb) {
    const int row = w * QW + rb * 32 + r32;
    const int64_t q = qbase + row;
    const char* prow = reinterpret_cast<const char*>(a.packed_queries) + (q < a.m ? q : 0) * (int64_t)RB;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      ahi[rb][j] = *reinterpret_cast<const u4x*>(prow + 16 * (2 * j + half));
      alo[rb][j] = *reinterpret_cast<const u4x*>(prow + 2 * KP + 16 * (2 * j + half));
    }
    myqn[rb] = q < a.m ? a.query_sqn[q] : 0.f;
    if (half == 1) set_thr(rb, tau_s[row]);
  }

  // Staging: chunk C of S steps is 4 S slots per row -- hi pieces 2 F .. 2 (F + S) - 1, then the lo pieces of the same
  // range -- at a row stride of 4 S + 1 slots; slot sigma of the buffer is row sigma / (4 S + 1), the stride's last slot
  // repeats the one before it.  Rows past n repeat row n - 1 and are masked by position.
  auto issue_chunk = [&](auto cc, int buf, int64_t t0) {
    constexpr int C = decltype(cc)::value;
    constexpr int S = pl_steps(NQ, C), F = pl_first(NQ, C), SPR = 4 * S + 1;
    for (int p = w; p < SPR; p += 4) {  // 64 rows x SPR slots = SPR wave passes of 64 x 16 bytes
      const int sigma = 64 * p + lane;
      const int row = sigma / SPR;
      const int s = min(sigma - row * SPR, 4 * S - 1);
      const int off = s < 2 * S ? 16 * (2 * F + s) : 2 * KP + 16 * (2 * F + s - 2 * S);
      const int64_t grow = min(t0 + row, a.n - 1);
      lds_dma16(ptrain + grow * (int64_t)RB + off, lds_offset(tile0 + buf * PL_BUF) + p * 1024);
    }
  };
  // staggered walk over the table (see knn_scan_long_kernel)
  const int64_t ntiles = (a.n - a.start + KNN_TN - 1) / KNN_TN;
  const int64_t tile_off = ((int64_t)blockIdx.x * 7919) % ntiles;
  auto tile_after = [&](int64_t t) { return t + 1 == ntiles ? (int64_t)0 : t + 1; };
  int64_t tcur = tile_off;
  issue_chunk(std::integral_constant<int, 0>{}, 0, a.start + tcur * KNN_TN);
  int buf = 0;
  int64_t next_drain = 0;
  for (int64_t tj = 0; tj < ntiles; ++tj, tcur = tile_after(tcur)) {
    const int64_t t0 = a.start + tcur * KNN_TN;
    f16x accs[RBN][KNN_TN / 32];
    pl_static_for(
        [&](auto cc) {
          constexpr int C = decltype(cc)::value;
          constexpr int S = pl_steps(NQ, C), F = pl_first(NQ, C), XSB = (4 * S + 1) * 16;
          __builtin_amdgcn_s_waitcnt(0);  // this wave's share of buffer `buf` has landed
          __syncthreads();                // ... everyone's has, and nobody still reads the other buffer
          // the next step of the (tile, chunk) sequence goes into the other buffer
          if constexpr (C + 1 < NCH) {
            issue_chunk(std::integral_constant<int, C + 1>{}, buf ^ 1, t0);
          } else {
            if (tj + 1 < ntiles) issue_chunk(std::integral_constant<int, 0>{}, buf ^ 1, a.start + tile_after(tcur) * KNN_TN);
          }
          const char* tl = tile0 + buf * PL_BUF;
#pragma unroll
          for (int ct = 0; ct < KNN_TN / 32; ++ct) {
            const char* xrow = tl + (ct * 32 + r32) * XSB;
            u4x bhi[S], blo[S];
#pragma unroll
            for (int j = 0; j < S; ++j) {
              bhi[j] = *reinterpret_cast<const u4x*>(xrow + 16 * (2 * j + half));
              blo[j] = *reinterpret_cast<const u4x*>(xrow + 16 * (2 * S + 2 * j + half));
            }
#pragma unroll
            for (int rb = 0; rb < RBN; ++rb) {
              f16x acc;
              if constexpr (C == 0) acc = f16x{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
              else acc = accs[rb][ct];
#pragma unroll
              for (int j = 0; j < S; ++j)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8x, ahi[rb][F + j]),
                                                              __builtin_bit_cast(bf8x, bhi[j]), acc, 0, 0, 0);
#pragma unroll
              for (int j = 0; j < S; ++j)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8x, ahi[rb][F + j]),
                                                              __builtin_bit_cast(bf8x, blo[j]), acc, 0, 0, 0);
#pragma unroll
              for (int j = 0; j < S; ++j)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8x, alo[rb][F + j]),
                                                              __builtin_bit_cast(bf8x, bhi[j]), acc, 0, 0, 0);
              accs[rb][ct] = acc;
            }
          }
          buf ^= 1;
        },
        std::make_integer_sequence<int, NCH>{});

    // ---- survivors, after the last chunk: any accumulator positive?  (as integers: v_max3_i32) ------------------------
    const int nvalid = (int)(a.n - t0 < (int64_t)KNN_TN ? a.n - t0 : (int64_t)KNN_TN);  // rows of this tile that exist
#pragma unroll
    for (int ct = 0; ct < KNN_TN / 32; ++ct) {
      const int col = ct * 32 + r32;
#pragma unroll
      for (int rb = 0; rb < RBN; ++rb) {
        const f16x acc = accs[rb][ct];
        int mx = max(__float_as_int(acc[0]), __float_as_int(acc[1]));
#pragma unroll
        for (int v = 2; v < 16; v += 2) mx = max(mx, max(__float_as_int(acc[v]), __float_as_int(acc[v + 1])));
        if (mx > 0 && col < nvalid) {
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            if (acc[v] > 0.f) {
              const int qslot = w * QW + rb * 32 + 8 * (v >> 2) + 4 * half + (v & 3);
              const int pos = atomicAdd(&q_cnt[qslot], 1);
              if (pos < KNN_CAP) q_i[qslot * KNN_CAP + pos] = (int)(t0 + col);
            }
          }
        }
      }
    }

    // ---- drain (wave-private state: no barrier): exact re-measurement of the survivors, then the k-best update -------
    // knn_scan_long_kernel's cadence; lane r merges the queue of the wave's query r into that query's list, round e
    // handles every lane's e-th entry (knn_scan_bf16x3_kernel's drain)
    if (tj < next_drain && tj + 1 < ntiles) continue;
    next_drain = tj + (tj < 64 ? 1 : tj < 256 ? 4 : tj < 1024 ? 8 : 16);
    const int qslot = w * QW + (lane < QW ? lane : 0);
    const int64_t q = qbase + qslot;
    int cnt = (lane < QW && q < a.m) ? q_cnt[qslot] : 0;
    if (!__any(cnt > 0)) continue;
    if (cnt > KNN_CAP) {
      a.overflow[q] = 1;
      cnt = KNN_CAP;
    }
    const int self = (cnt > 0 && a.self_idx) ? (int)a.self_idx[q] : -1;
    const float* qrow = a.queries + (q < a.m ? q : 0) * (int64_t)d;
    float* ld = a.best_d + (q < a.m ? q : 0) * (int64_t)k;
    int* li = a.best_i + (q < a.m ? q : 0) * (int64_t)k;
    float tau = tau_s[qslot];
    const int rounds = wave_max(cnt);
    for (int e = 0; e < rounds; ++e) {
      if (e < cnt) {
        const int ci = q_i[qslot * KNN_CAP + e];
        if (ci != self) {
          const float* xrow = a.train + ci * (int64_t)d;
          float cd = 0.f;
          for (int c = 0; c < d; c += 4) {
            const f4x df = *reinterpret_cast<const f4x*>(qrow + c) - *reinterpret_cast<const f4x*>(xrow + c);
            cd += df.x * df.x + df.y * df.y + df.z * df.z + df.w * df.w;
          }
          if (cd < tau) {
            // one pass over the list, in blocks of loads that are all in flight together: its largest entry (replaced)
            // and its second largest (the new tau, or cd)
            float m1 = -__builtin_inff(), m2 = -__builtin_inff();
            int at = 0;
            for (int j0 = 0; j0 < k; j0 += PL_SCAN_BLOCK) {
              float lv[PL_SCAN_BLOCK];
#pragma unroll
              for (int u = 0; u < PL_SCAN_BLOCK; ++u) lv[u] = ld[min(j0 + u, k - 1)];
#pragma unroll
              for (int u = 0; u < PL_SCAN_BLOCK; ++u) {
                const float v = j0 + u < k ? lv[u] : -__builtin_inff();
                if (v > m1) {
                  m2 = m1;
                  m1 = v;
                  at = j0 + u;
                } else if (v > m2) {
                  m2 = v;
                }
              }
            }
            ld[at] = cd;
            li[at] = ci;
            tau = fmaxf(m2, cd);
          }
        }
      }
    }
    if (cnt > 0) {
      tau_s[qslot] = tau;
      q_cnt[qslot] = 0;
    }
    __builtin_amdgcn_s_waitcnt(0);
    if (half == 1) {
#pragma unroll
      for (int rb = 0; rb < RBN; ++rb) set_thr(rb, tau_s[w * QW + rb * 32 + r32]);
    }
  }
}

template <int NQ>
static int launch_knn_prefilter_long_nq(const KnnPackedArgs& a, hipStream_t stream) {
  constexpr int RBN = pl_rbn(NQ);
  constexpr size_t lds = pl_lds_bytes(RBN);
  static_assert(lds <= 64 * 1024, "no opt-in needed");
  const int64_t grid = (a.m + KNN_QB * RBN - 1) / (KNN_QB * RBN);
  hipLaunchKernelGGL((knn_prefilter_long_kernel<NQ, RBN>), dim3((unsigned)grid), dim3(256), lds, stream, a);
  MGP_HIP_CHECK_LAUNCH();
  return MGP_OK;
}

static int launch_knn_prefilter_long(const KnnPackedArgs& a, hipStream_t stream) {
  if (a.k < 1 || a.k > 64 || a.d % 4 != 0 || a.d <= 64 || a.d > KNN_LONG_MAX_D) return MGP_EUNSUPPORTED;
  const uintptr_t al = (uintptr_t)a.train | (uintptr_t)a.queries | (uintptr_t)a.packed_train | (uintptr_t)a.packed_queries;
  if (al % 16 != 0) return MGP_EUNSUPPORTED;
  if (a.n >= (int64_t)1 << 31) return MGP_EUNSUPPORTED;  // list indices are 32-bit
  if ((a.m + KNN_QB - 1) / KNN_QB >= (int64_t)1 << 31) return MGP_EUNSUPPORTED;
  switch ((a.d + 2 + 15) / 16) {  // features + the two threshold slots, in matrix steps
    case 5: return launch_knn_prefilter_long_nq<5>(a, stream);
    case 6: return launch_knn_prefilter_long_nq<6>(a, stream);
    case 7: return launch_knn_prefilter_long_nq<7>(a, stream);
    case 8: return launch_knn_prefilter_long_nq<8>(a, stream);
    case 9: return launch_knn_prefilter_long_nq<9>(a, stream);
    case 10: return launch_knn_prefilter_long_nq<10>(a, stream);
    case 11: return launch_knn_prefilter_long_nq<11>(a, stream);
    case 12: return launch_knn_prefilter_long_nq<12>(a, stream);
    case 13: return launch_knn_prefilter_long_nq<13>(a, stream);
    case 14: return launch_knn_prefilter_long_nq<14>(a, stream);
    case 15: return launch_knn_prefilter_long_nq<15>(a, stream);
    case 16: return launch_knn_prefilter_long_nq<16>(a, stream);
    default: return launch_knn_prefilter_long_nq<17>(a, stream);
  }
}

}  // namespace mgp

extern "C" {

int mgp_knn_scan_long_bf16x3(const float* train, const void* packed_train, const float* train_sqn, int64_t n, int d,
                             const float* queries, const void* packed_queries, const float* query_sqn,
                             const int64_t* self_idx, int64_t m, int k, int64_t start, float* best_d, int32_t* best_i,
                             int32_t* overflow, void* st) {
  if (n < 0 || m < 0 || d < 1 || k < 1 || start < 0) return MGP_EINVAL;
  if (m == 0 || start >= n) return MGP_OK;
  if (!train || !packed_train || !train_sqn || !queries || !packed_queries || !query_sqn || !best_d || !best_i || !overflow)
    return MGP_EINVAL;
  mgp::KnnPackedArgs a{train, packed_train, train_sqn, queries, packed_queries, query_sqn, self_idx, best_d, best_i,
                       overflow, n, m, start, d, k};
  return mgp::launch_knn_prefilter_long(a, static_cast<hipStream_t>(st));
}

}  // extern "C"
