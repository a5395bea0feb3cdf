// MFMA GEMM for gfx950: C[m,n] = epi(sum_k A[m,k] W[n,k]).
//
//  * operands bf16 (v_mfma_f32_16x16x32_bf16), e4m3 (v_mfma_f32_16x16x32_fp8_fp8) or f32 (v_mfma_f32_16x16x4_f32,
//    exact fp32), fp32 accumulate;
//  * tile BM x BN x 128 bytes of K, WM x WN waves; two data paths for the K tiles (gemm_glds_kernel): LDS-DMA into an
//    NS-stage ring, or register staging into two LDS stages (STG) -- the tile rule in plan_gemm picks per launch;
//  * both operands are K-contiguous; a 16-byte chunk per lane is the unit everywhere:
//      global -> LDS (16 B/lane, 8 lanes cover one 128-B row = full cache lines), chunk XOR-swizzle
//      phys = chunk ^ ((row >> 1) & 7), applied on the source address for LDS-DMA
//      LDS -> fragments with ds_read_b128 at (row = lane & 15, chunk = kstep*4 + (lane >> 4)),
//    conflict-free for 128-byte rows.  One chunk feeds one bf16 MFMA (K=32 across the 4 lane groups), two e4m3
//    MFMAs or four f32 MFMAs (the k permutation is the same for both operands, so the sum is unchanged);
//  * operands are swapped (first = W rows, second = A rows) so each lane ends up with 4 consecutive
//    n for one m: bias / LayerScale / residual / output move as 8- or 16-byte vectors;
//  * the A loader is either a plain row-major matrix or an implicit 3x3 (pad 1, stride 1|2)
//    convolution over an NHWC activation, with optional ReLU-on-load (pre-activation units); stride-1 convs on
//    the large maps use conv3_halo_kernel (input tile resident in LDS) instead.
#include "gemm_epi.h"
#include "linear_site.h"
#include <cstdio>
#include <deque>
#include <vector>

namespace d2s {

// ================================================================================================
// LDS-DMA ring.  The K tiles travel
// global -> LDS directly (global_load_lds_dwordx4, 1 KiB per wave-instruction, no staging VGPRs, no
// ds_write pass) into a ring of NS stages, PD = NS-1 tiles ahead, with counted vmcnt and ONE raw
// s_barrier per tile:
//     wait my loads of tile t (vmcnt <= (PD-1) tiles in flight)  ->  s_barrier  (all loads of t
//     landed AND everybody finished computing t-1)  ->  issue tile t+PD into the stage t-1 used
//     ->  compute t.
// LDS-DMA writes lane-linear (base + lane*16), so the XOR swizzle moves to the SOURCE address:
// the lane that owns LDS slot (row r, phys chunk p) fetches global chunk p ^ ((r>>1)&7)
// (cdna_hip_programming.md rule 21: linear dest + swizzled source + swizzled read).
// Out-of-range rows / K tail / conv padding fetch from a zero page.  ReLU-on-load is applied when
// the A fragments are read (v_pk_max_i16 for bf16).
// ================================================================================================
__device__ u32x4 d2s_zero_page[4];

// tuning aid (build with D2S_HIPCC_DEFS=-DD2S_GLDS_TIMING): thread 0 of every block of gemm_glds_kernel stamps the 100 MHz wall
// clock at entry / ring primed / first K tile landed / K loop done / epilogue done; tools/glds_timeline.py reads them
#ifdef D2S_GLDS_TIMING
__device__ unsigned long long glds_timing[4096 * 8];
#define GL_STAMP(SLOT) { if (threadIdx.x == 0 && blockIdx.y == 0 && blockIdx.x < 4096) glds_timing[blockIdx.x * 8 + (SLOT)] = wall_clock64(); }
#else
#define GL_STAMP(SLOT) {}
#endif

// max(x, floor) on a fragment: floor = 0 gives ReLU, floor = lowest gives identity (no branch in the MFMA stream).  The bf16 form is
// in gemm_epi.h (the convolutions of conv3.hip use it too).
__device__ __forceinline__ u32x4 relu_frag(u32x4 v, int, fp8_t) { return v; }
__device__ __forceinline__ u32x4 relu_frag(u32x4 v, int, bx3_t) { return v; }   // bf16x3: ReLU-on-load happens on the fp32 values as they are staged   // e4m3 operands: encoder linears only, no ReLU-on-load
__device__ __forceinline__ u32x4 relu_frag(u32x4 v, int floor_bits, float) {
    f32x4 x = __builtin_bit_cast(f32x4, v);
    float f = floor_bits == 0 ? 0.f : -3.0e38f;
    x = __builtin_elementwise_max(x, (f32x4){f, f, f, f});
    return __builtin_bit_cast(u32x4, x);
}

template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// chunk XOR for a row of CPR chunks: conflict-free ds_read_b128 for 128-byte (CPR 8) and 256-byte (CPR 16) rows
// (64-byte rows, CPR 4: rows r and r+2 share banks -> XOR by (r >> 1) & 3)
template <int CPR> __device__ __forceinline__ int swz_row(int r) { return CPR == 8 ? ((r >> 1) & 7) : (CPR == 4 ? ((r >> 1) & 3) : (r & 15)); }

// STG = true: register-staged variant of the same tile.  The K tile travels global -> VGPRs (global_load_dwordx4)
// -> LDS (ds_write_b128, same lane-linear slots as the LDS-DMA path, so fragment reads are unchanged) with TWO LDS
// stages: at the top of iteration t (after the barrier) the registers holding tile t+1 -- loaded during compute(t-1)
// -- are written to the stage compute(t-1) just released, the loads of tile t+2 are issued, then tile t is computed.
// Measured on this chip (tools/ubench/l2_to_lds): L2-resident data reaches LDS at ~27 TB/s through VGPRs vs
// ~13-16 TB/s by LDS-DMA, and the freed LDS (2 stages instead of 3) admits the 256 x 256 tile.
// (An intra-block split-K variant -- several wave groups per block, each running the pipeline over every KG-th K tile,
// accumulators summed through LDS -- was built and swept at batch 1: the batch-1 launches are L2->LDS-bandwidth-bound
// (~10 TB/s aggregate), not latency-bound; it won 9 % on FC2 in isolation and lost 2 % in the pipeline.  Removed.)
// both kernels of this file that warm their argument lines (KERNARG_WARM, common.h: one dword of every 64-byte line up to 0x140) carry
// at least a GemmA and a GemmEpi by value behind >= 8 bytes of scalars
static_assert(sizeof(GemmA) + sizeof(GemmEpi) + 8 >= KERNARG_WARM_BYTES, "KERNARG_WARM reads past the kernarg segment");
template <typename T, int BM, int BN, int WM, int WN, int NS, int CPR, int STG = 0>
__global__ void __launch_bounds__(64 * WM * WN)
gemm_glds_kernel(const T* __restrict__ W, const void* a_ptr, long a_lda, int M, int N, int K, int Kpad, int xn, GemmA a, GemmEpi e) {
    // Argument order: what the tile map and the first operand requests need -- 11 dwords -- comes first, so that the hardware's kernarg
    // PRELOAD (gfx950: the first 16 dwords arrive in SGPRs with the wave; -mllvm -amdgpu-kernarg-preload-count=16, build.py) covers
    // it: the lean (latency-regime) instantiations request their first K tiles before any kernarg load has returned.  a_ptr / a_lda
    // repeat a.ptr / a.lda for that purpose.
    // STG: 0 = LDS-DMA ring, every loader; 1 = register-staged, two LDS stages; 2 = "lean" LDS-DMA ring: descriptor-addressed plain
    // linears only (a.buf guaranteed by the launcher) -- the pointer / implicit-conv loaders and their per-row set-up are compiled out
    static_assert(STG == 0 || STG == 2 || (STG == 1 && NS == 2), "the register-staged variant uses two LDS stages");
    constexpr bool LEAN = STG == 2;
    constexpr bool BX3 = std::is_same<T, bx3_t>::value;   // A: fp32 in memory, split hi / lo when the staging registers are stored
    static_assert(!BX3 || CPR == 8, "bf16x3 units are laid out for 128-byte K tiles");
    // (bf16x3 with STG == 0: both operands already in the unit format, LDS-DMA like any other type; STG == 1: A is fp32)
    constexpr int CE = Prec<T>::CE;
    constexpr int BK = CPR * CE;                    // K tile: CPR 16-byte chunks per row (8 -> 128 B, 16 -> 256 B)
    constexpr int RPI = 64 / CPR;                   // rows covered by one 1-KiB LDS-DMA wave-instruction
    constexpr int NW = WM * WN;                     // waves per block
    constexpr int AI = BM / (RPI * NW), BI = BN / (RPI * NW);   // LDS-DMA instructions per thread per tile (A / W)
    constexpr int LPT = AI + BI;
    constexpr int FM = BM / WM / 16, FN = BN / WN / 16;   // 16x16 fragments per wave
    constexpr int PD = NS - 1;
    constexpr int STAGE = (BM + BN) * CPR;          // chunks per stage
    __shared__ __attribute__((aligned(16))) u32x4 lds[NS * STAGE];
    KERNARG_WARM(kaw_)                               // every 64-byte line of the ~390 argument bytes in one round trip (common.h)
    if constexpr (STG != 2) { KERNARG_WARM_END(kaw_) }   // (lean: waited for behind the first operand requests)
    D2S_POISON_LDS(lds, NS * STAGE)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wid / WN, wave_n = wid % WN;
    int tm_, tn_;
    GL_STAMP(0)
    if (!tile_of_block(blockIdx.x, (M + BM - 1) / BM, (N + BN - 1) / BN, xn, tm_, tn_)) return;
    const int bm0 = tm_ * BM, bn0 = tn_ * BN;
    // this lane's slot inside a 64-slot wave-instruction: row lane/CPR of RPI, phys chunk lane%CPR;
    // its source chunk is the same for every instruction i (rows differ by multiples of RPI*NW,
    // which the row swizzle's period divides)
    static_assert((RPI * NW) % 16 == 0, "row swizzle must be invariant across a thread's instructions");
    static_assert(BM % (RPI * NW) == 0 && BN % (RPI * NW) == 0 && BM % (16 * WM) == 0 && BN % (16 * WN) == 0, "tile must split evenly over the waves");
    const int lrow = wid * RPI + lane / CPR;
    const int src_chunk = (lane % CPR) ^ swz_row<CPR>(lrow);
    const T* zero = (const T*)d2s_zero_page;

    const T* arow[AI];
    int aiy[AI], aix[AI];
    bool aok[AI];
    if constexpr (!LEAN)
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        int m = bm0 + i * NW * RPI + lrow;
        aok[i] = m < M;
        int mm = aok[i] ? m : 0;
        if (a.mode == A_PLAIN) { arow[i] = (const T*)a.ptr + (long)mm * a.lda; aiy[i] = aix[i] = 0; }
        else {
            int ox = mm % a.Wo, oy = (mm / a.Wo) % a.Ho, b = mm / (a.Wo * a.Ho);
            aiy[i] = oy * a.stride - 1; aix[i] = ox * a.stride - 1;
            arow[i] = (const T*)a.ptr + (long)b * a.Hi * a.Wi * a.C;
        }
    }
    const T* wrow = W + (long)(bn0 + lrow) * Kpad + src_chunk * CE;
    const float inv_c = a.mode == A_CONV3 ? 1.0f / (float)a.C : 0.f;
    // Plain linears (a.buf, LDS-DMA path): both operands through buffer descriptors.  The per-lane byte offsets below are fixed
    // for the whole K loop and a K tile is ONE scalar offset -- no 64-bit address arithmetic, bounds selects or zero-page
    // pointers per load (at batch 1 that was ~20 VALU + ~20 SALU per K tile next to 4 MFMAs).  Rows past M get an offset past
    // every descriptor's range: the hardware returns zeros for them.
    constexpr int ES = (int)sizeof(T);
    // (descriptors are built unconditionally -- a few scalar instructions; the offsets only where the path is taken)
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(a_ptr), 0, (unsigned)((long)M * a_lda * ES), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc(uniform_ptr(W), 0, (unsigned)((long)((N + 255) / 256 * 256) * Kpad * ES), 0x00020000);
    unsigned voA[AI], voW[BI];
    if constexpr (STG != 1) {
        if (LEAN || a.buf) {
#pragma unroll
            for (int i = 0; i < AI; ++i) {
                const int m = bm0 + i * NW * RPI + lrow;
                voA[i] = m < M ? (unsigned)((long)m * a_lda * ES) + (unsigned)(src_chunk * 16) : 0x80000000u;
            }
#pragma unroll
            for (int i = 0; i < BI; ++i) voW[i] = (unsigned)((long)(bn0 + lrow + RPI * NW * i) * Kpad * ES) + (unsigned)(src_chunk * 16);
        }
    }
#define D2S_ISSUE_BUF(KT)                                                                                        \
    {                                                                                                            \
        u32x4* st_ = lds + ((KT) % NS) * STAGE;                                                                  \
        const int so_ = ((KT) + kt0) * (BK * ES);                                                                \
        _Pragma("unroll") for (int i = 0; i < AI; ++i) lds_dma16(rsA, st_ + (i * NW + wid) * 64, voA[i], so_);    \
        _Pragma("unroll") for (int i = 0; i < BI; ++i) lds_dma16(rsW, st_ + BM * CPR + (i * NW + wid) * 64, voW[i], so_); \
    }

    // lean instantiations (one K range per block: the launcher never splits K for them): the ring is primed HERE, from preloaded
    // arguments only; everything that reads the rest of the kernarg segment (LayerNorm statistics, epilogue set-up) comes after
    if constexpr (LEAN) {
        constexpr int kt0 = 0;
        const int nkt_ = (K + BK - 1) / BK;
#pragma unroll
        for (int t = 0; t < PD; ++t)
            if (t < nkt_) D2S_ISSUE_BUF(t)
        KERNARG_WARM_END(kaw_)
    }

    // D2S_MOVE(slot index, source, LDS destination): LDS-DMA straight into the ring, or a load into staging registers
    u32x4 stg[1][STG == 1 ? LPT : 1];
#define D2S_MOVE(S, IDX, SRC, DST)                                                                                \
    do {                                                                                                         \
        if constexpr (STG == 1) stg[S][IDX] = *(const u32x4*)(SRC);                                                 \
        else __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(SRC),             \
                                              (__attribute__((address_space(3))) void*)(DST), 16, 0, 0);         \
    } while (0)
#define D2S_ISSUE_TILE(KT, S)                                                                                    \
    {                                                                                                            \
        u32x4* st_ = lds + ((KT) % NS) * STAGE;                                                                  \
        const int k_ = ((KT) + kt0) * BK + src_chunk * CE;                                                       \
        if (a.mode == A_PLAIN) {                                                                                 \
            _Pragma("unroll") for (int i = 0; i < AI; ++i) {                                                     \
                const T* s_ = (aok[i] && k_ < K) ? arow[i] + k_ : zero;                                          \
                D2S_MOVE(S, i, s_, st_ + (i * NW + wid) * 64);                                                    \
            }                                                                                                    \
        } else {                                                                                                 \
            int tap_ = (int)(((float)k_ + 0.5f) * inv_c);                                                        \
            int c0_ = k_ - tap_ * a.C;                                                                           \
            int ky_ = tap_ / 3, kx_ = tap_ - ky_ * 3;                                                            \
            _Pragma("unroll") for (int i = 0; i < AI; ++i) {                                                     \
                int iy_ = aiy[i] + ky_, ix_ = aix[i] + kx_;                                                      \
                bool ok_ = aok[i] && k_ < K && iy_ >= 0 && iy_ < a.Hi && ix_ >= 0 && ix_ < a.Wi;                 \
                const T* s_ = ok_ ? arow[i] + ((long)iy_ * a.Wi + ix_) * a.C + c0_ : zero;                       \
                D2S_MOVE(S, i, s_, st_ + (i * NW + wid) * 64);                                                    \
            }                                                                                                    \
        }                                                                                                        \
        _Pragma("unroll") for (int i = 0; i < BI; ++i)                                                           \
            D2S_MOVE(S, AI + i, wrow + (long)(RPI * NW * i) * Kpad + ((KT) + kt0) * BK, st_ + BM * CPR + (i * NW + wid) * 64); \
    }
    // staging registers -> LDS, the same lane-linear slots the LDS-DMA path fills.  bf16x3: this lane's A chunk is 4 fp32 values
    // (logical chunk c = src_chunk of the row's K tile): their bf16 hi / lo pieces are the (c & 1) halves of the hi / lo chunk of
    // unit c >> 1, i.e. logical chunks 2 (c >> 1) and 2 (c >> 1) + 1, swizzled like every other chunk of the row.
    const int bx_row = (lane / CPR) * CPR, bx_sw = swz_row<CPR>(lrow);
    const int bx_hi = (bx_row + (((src_chunk >> 1) * 2) ^ bx_sw)) * 2 + (src_chunk & 1);           // in 8-byte units
    const int bx_lo = (bx_row + (((src_chunk >> 1) * 2 + 1) ^ bx_sw)) * 2 + (src_chunk & 1);
#define D2S_STORE_STG(KT, S)                                                                                     \
    {                                                                                                            \
        u32x4* st_ = lds + ((KT) % NS) * STAGE;                                                                  \
        if constexpr (BX3) {                                                                                     \
            _Pragma("unroll") for (int i = 0; i < AI; ++i) {                                                     \
                f32x4 x_ = __builtin_bit_cast(f32x4, stg[S][i]);                                                 \
                if (a.relu) x_ = __builtin_elementwise_max(x_, (f32x4){0.f, 0.f, 0.f, 0.f});                     \
                uint2 h_, l_;                                                                                    \
                bx3_split4(x_, h_, l_);                                                                          \
                uint2* s2_ = (uint2*)(st_ + (i * NW + wid) * 64);                                                \
                s2_[bx_hi] = h_; s2_[bx_lo] = l_;                                                                \
            }                                                                                                    \
        } else {                                                                                                 \
            _Pragma("unroll") for (int i = 0; i < AI; ++i) st_[(i * NW + wid) * 64 + lane] = stg[S][i];          \
        }                                                                                                        \
        _Pragma("unroll") for (int i = 0; i < BI; ++i) st_[BM * CPR + (i * NW + wid) * 64 + lane] = stg[S][AI + i]; \
    }

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // split-K (e.ksplit > 1): blockIdx.y owns a contiguous range of K tiles and writes raw fp32 partials
    const int nkt_all = (K + BK - 1) / BK;
    const int ksplit = LEAN ? 1 : (e.ksplit > 1 ? e.ksplit : 1);
    const int kt0 = (int)(((long)nkt_all * blockIdx.y) / ksplit);
    const int nkt = (int)(((long)nkt_all * (blockIdx.y + 1)) / ksplit) - kt0;
    const int fr = lane & 15, fg = lane >> 4;
    // LN-folded consumer: the producer left (sum, sum of squares) per row and column block in e.ln_stats[slot][M][2].
    // The 4 lane groups of a row share the slots (slot = fg + 4q); the loads are issued here, before the K loop, and
    // summed after it.  (Registers, not LDS: a second __shared__ object makes the compiler track the LDS-DMA writes
    // and put s_waitcnt vmcnt(0) in front of every fragment read.)
    constexpr bool LN_ON = WN > 1;                  // the WN == 1 (fused-head) tiles never see an LN-folded linear
    constexpr int LNS = LN_ON ? 4 : 1;              // <= 16 column blocks
    float2 lnp[FM][LNS];
    if (LN_ON && e.ln_stats) {
#pragma unroll
        for (int i = 0; i < FM; ++i) {
            const int m = bm0 + wave_m * (BM / WM) + i * 16 + fr;
#pragma unroll
            for (int q = 0; q < LNS; ++q) {
                const int sl = fg + 4 * q;
                lnp[i][q] = (m < M && sl < e.ln_slots) ? ((const float2*)e.ln_stats)[(long)sl * (e.ln_M ? e.ln_M : M) + m] : make_float2(0.f, 0.f);
            }
        }
    }
    // RELU is a literal: the K loop exists twice (with / without ReLU-on-load) so that plain linears do not pay
    // 4 v_pk_max per A fragment (a third of the loop's VALU work) for an identity
#define D2S_COMPUTE(KT, RELU)                                                                                    \
    {                                                                                                            \
        const u32x4* A_l = lds + ((KT) % NS) * STAGE + (wave_m * (BM / WM)) * CPR;                               \
        const u32x4* B_l = lds + ((KT) % NS) * STAGE + BM * CPR + (wave_n * (BN / WN)) * CPR;                    \
        if constexpr (BX3) {                                                                                     \
            /* one K = 32 step per 128-byte tile: lane group fg takes unit BX3_UNIT(fg) = chunks 2 u (hi), 2 u + 1 (lo) */ \
            const int cu_ = 2 * BX3_UNIT(fg);                                                                    \
            u32x4 fbh[FN], fbl[FN];                                                                              \
            _Pragma("unroll") for (int j = 0; j < FN; ++j) {                                                     \
                int r = j * 16 + fr; fbh[j] = B_l[r * CPR + (cu_ ^ swz_row<CPR>(r))]; fbl[j] = B_l[r * CPR + ((cu_ + 1) ^ swz_row<CPR>(r))]; \
            }                                                                                                    \
            _Pragma("unroll") for (int i = 0; i < FM; ++i) {                                                     \
                int r = i * 16 + fr;                                                                             \
                const u32x4 fah = A_l[r * CPR + (cu_ ^ swz_row<CPR>(r))], fal = A_l[r * CPR + ((cu_ + 1) ^ swz_row<CPR>(r))]; \
                _Pragma("unroll") for (int j = 0; j < FN; ++j) mma_bx3(acc[i][j], fbh[j], fbl[j], fah, fal);     \
            }                                                                                                    \
        } else {                                                                                                 \
        _Pragma("unroll") for (int ks = 0; ks < CPR / 4; ++ks) {                                                 \
            /* W fragments stay live for the k-step; A fragments stream through one at a time */                 \
            /* (keeps the 8-wave 256-row tiles inside the 256-register budget) */                                \
            u32x4 fb[FN];                                                                                        \
            _Pragma("unroll") for (int j = 0; j < FN; ++j) {                                                     \
                int r = j * 16 + fr; fb[j] = B_l[r * CPR + ((ks * 4 + fg) ^ swz_row<CPR>(r))];                   \
            }                                                                                                    \
            _Pragma("unroll") for (int i = 0; i < FM; ++i) {                                                     \
                int r = i * 16 + fr;                                                                             \
                u32x4 fa = A_l[r * CPR + ((ks * 4 + fg) ^ swz_row<CPR>(r))];                                     \
                if (RELU) fa = relu_frag(fa, 0, T());                                                            \
                _Pragma("unroll") for (int j = 0; j < FN; ++j) mma_chunk(acc[i][j], fb[j], fa, T());             \
            }                                                                                                    \
        }                                                                                                        \
        }                                                                                                        \
    }
#define D2S_K_LOOP(RELU)                                                                                         \
    if constexpr (STG == 1) {                                                                                    \
        for (int kt = 0; kt < nkt; ++kt) {                                                                       \
            __syncthreads();       /* tile kt visible, stage (kt+1)&1 released, my loads of kt+1 landed */        \
            if (kt + 1 < nkt) D2S_STORE_STG(kt + 1, 0)                                                           \
            if (kt + 2 < nkt) D2S_ISSUE_TILE(kt + 2, 0)                                                          \
            D2S_COMPUTE(kt, RELU)                                                                                \
        }                                                                                                        \
    } else {                                                                                                     \
        for (int kt = 0; kt < nkt; ++kt) {                                                                       \
            /* tiles kt .. min(kt+PD-1, nkt-1) are in flight; let all but tile kt stay in flight */              \
            if (kt + PD - 1 < nkt) wait_vmcnt<(PD - 1) * LPT>();                                                 \
            else wait_vmcnt<0>();                                                                                \
            __builtin_amdgcn_s_barrier();                                                                        \
            if (kt + PD < nkt) D2S_ISSUE_TILE(kt + PD, 0)                                                        \
            D2S_COMPUTE(kt, RELU)                                                                                \
        }                                                                                                        \
    }
    bool done_buf = false;
    if constexpr (STG != 1) {
        if (LEAN || a.buf) {                         // plain linear, descriptor-addressed ring (same ring, same waits)
            if constexpr (!LEAN) {
#pragma unroll
                for (int t = 0; t < PD; ++t)
                    if (t < nkt) D2S_ISSUE_BUF(t)
            }
            GL_STAMP(1)
            for (int kt = 0; kt < nkt; ++kt) {
                if (kt + PD - 1 < nkt) wait_vmcnt<(PD - 1) * LPT>();
                else wait_vmcnt<0>();
                __builtin_amdgcn_s_barrier();
                if (kt == 0) { GL_STAMP(2) }
                if (kt + PD < nkt) D2S_ISSUE_BUF(kt + PD)
                D2S_COMPUTE(kt, 0)
            }
            done_buf = true;
        }
    }
    if constexpr (!LEAN)
    if (!done_buf) {
    if constexpr (STG == 1) {
        if (nkt > 0) { D2S_ISSUE_TILE(0, 0) D2S_STORE_STG(0, 0) }
        if (nkt > 1) D2S_ISSUE_TILE(1, 0)
    } else {
#pragma unroll
        for (int t = 0; t < PD; ++t)
            if (t < nkt) D2S_ISSUE_TILE(t, 0)
    }
    if (a.relu) { D2S_K_LOOP(1) } else { D2S_K_LOOP(0) }
    }
    GL_STAMP(3)
#undef D2S_ISSUE_BUF
#undef D2S_K_LOOP
#undef D2S_COMPUTE
#undef D2S_ISSUE_TILE
#undef D2S_STORE_STG
#undef D2S_MOVE

    // MAP_HEAD: the DPT head's tail fused into conv2 -- depth[m] = relu(b3 + sum_n w3[n] * relu(acc[m][n] + bias[n]))
    // (HF DepthAnythingDepthEstimationHead: conv2 -> ReLU -> conv3 (1x1, C->1) -> ReLU).  One wave owns all N
    // columns of its rows (WN == 1, N <= BN), so the channel sum is registers + two cross-lane-group shuffles.
    if constexpr (WN == 1) {
        if (e.map == MAP_HEAD) {
            static_for<FM>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                const int m = bm0 + wave_m * (BM / WM) + i * 16 + fr;
                float s = 0.f;
                static_for<FN>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    const int n0 = j * 16 + fg * 4;
                    if (n0 < N) {
                        float b[4], w[4];
                        load4(e.bias + n0, b); load4(e.scale + n0, w);
                        s += fmaxf(acc[i][j][0] + b[0], 0.f) * w[0] + fmaxf(acc[i][j][1] + b[1], 0.f) * w[1] +
                             fmaxf(acc[i][j][2] + b[2], 0.f) * w[2] + fmaxf(acc[i][j][3] + b[3], 0.f) * w[3];
                    }
                });
                s += __shfl_xor(s, 16);
                s += __shfl_xor(s, 32);
                if (fg == 0 && m < M) ((float*)e.out)[m] = head_activation(s + e.head_b3, e.head_max_depth);
            });
            return;
        }
    }

    float2 ln_s[FM];
    float ln_cs[FN][4];                             // colsum(W') of this lane's columns: independent of the row fragment
    if (LN_ON && e.ln_csum) {
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            const int n0 = bn0 + wave_n * (BN / WN) + j * 16 + fg * 4;
            if (n0 < N) load4(e.ln_csum + n0, ln_cs[j]);
            else { ln_cs[j][0] = ln_cs[j][1] = ln_cs[j][2] = ln_cs[j][3] = 0.f; }
        }
    }
    // Latency regime only (the lean instantiations, every block resident): column vectors and residual values of all the wave's
    // fragments are requested before the first store (gemm_epi.h, epi_res1_load).  In the throughput tiles the extra registers
    // cost resident waves (64 x 128: 70 -> 100 VGPRs, 6 -> 4 waves / SIMD; batch 4: -12 % frames/s, measured) and the other
    // waves cover the round trips anyway.
    constexpr bool PRE = STG == 2 && FM * FN <= 8;
    EpiCols cols[PRE ? FN : 1];
    if constexpr (PRE) {
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            const int n0 = bn0 + wave_n * (BN / WN) + j * 16 + fg * 4;
            if (n0 < N) epi_cols_load(e, n0, cols[j]);
        }
    }
    float pre[PRE ? FM : 1][PRE ? FN : 1][4];
    const bool pre_on = PRE && ksplit == 1 && epi_res1_ahead(e);
    if constexpr (PRE) {
        if (pre_on) {
            static_for<FM>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                const int m = bm0 + wave_m * (BM / WM) + i * 16 + fr;
                static_for<FN>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    const int n0 = bn0 + wave_n * (BN / WN) + j * 16 + fg * 4;
                    if (m < M && n0 < N) epi_res1_load<T>(e, m, n0, pre[i][j]);
                });
            });
        }
    }
    // compile-time indices (a plain `#pragma unroll` over this large body is not honoured for the
    // 32-fragment tiles, and a run-time index would put the accumulators in scratch)
    static_for<FM>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const int m = bm0 + wave_m * (BM / WM) + i * 16 + fr;
        float s1 = 0.f, s2 = 0.f;                  // LN-folded producer: this lane's share of the row's sum / sum of squares
        float ln_mean = 0.f, ln_rstd = 1.f;
        if (LN_ON && e.ln_csum) {
            float t1 = (lnp[i][0].x + lnp[i][1 % LNS].x) + (lnp[i][2 % LNS].x + lnp[i][3 % LNS].x);
            float t2 = (lnp[i][0].y + lnp[i][1 % LNS].y) + (lnp[i][2 % LNS].y + lnp[i][3 % LNS].y);
            t1 += __shfl_xor(t1, 16); t2 += __shfl_xor(t2, 16);
            t1 += __shfl_xor(t1, 32); t2 += __shfl_xor(t2, 32);
            ln_mean = t1 / (float)e.ln_dim;
            ln_rstd = rsqrtf(fmaxf(t2 / (float)e.ln_dim - ln_mean * ln_mean, 0.f) + e.ln_eps);
        }
        if (m < M) {
            static_for<FN>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                const int n0 = bn0 + wave_n * (BN / WN) + j * 16 + fg * 4;
                if (n0 < N) {
                    float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                    if (ksplit > 1) store4(e.part + ((long)blockIdx.y * M + m) * N + n0, v);     // reduced by splitk_reduce_kernel
                    else {
                        const bool ln = LN_ON && e.ln_csum != nullptr;
                        if (ln) {
                            if (e.deq) { float q[4]; load4(e.deq + n0, q); v[0] *= q[0]; v[1] *= q[1]; v[2] *= q[2]; v[3] *= q[3]; }   // e4m3 operands -> real units first
                            v[0] = ln_rstd * (v[0] - ln_mean * ln_cs[j][0]); v[1] = ln_rstd * (v[1] - ln_mean * ln_cs[j][1]);
                            v[2] = ln_rstd * (v[2] - ln_mean * ln_cs[j][2]); v[3] = ln_rstd * (v[3] - ln_mean * ln_cs[j][3]);
                        }
                        epilogue_dispatch<T>(e, m, n0, v, ln, PRE && pre_on ? pre[PRE ? i : 0][PRE ? j : 0] : nullptr, PRE ? &cols[PRE ? j : 0] : nullptr);
                        s1 += (v[0] + v[1]) + (v[2] + v[3]);
                        s2 += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
                    }
                }
            });
        }
        if (LN_ON && e.stats_out) {                 // the 4 lane groups of a row hold 4 columns each of every fragment
            s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16);
            s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
            ln_s[i] = make_float2(s1, s2);
        }
    });
    if (LN_ON && e.stats_out) {
        // the block's WN waves cover BN columns of the same rows: add them up through the (now idle) stage memory so the
        // consumer reads one partial per column block.  Fixed order -> bit-reproducible.
        float2* red = (float2*)lds;
        __syncthreads();                            // every wave is done reading its last fragments
#pragma unroll
        for (int i = 0; i < FM; ++i)
            if (fg == 0) red[wave_n * BM + wave_m * (BM / WM) + i * 16 + fr] = ln_s[i];
        __syncthreads();
        for (int r = tid; r < BM; r += 64 * NW) {
            float2 t = red[r];
            for (int w = 1; w < WN; ++w) { t.x += red[w * BM + r].x; t.y += red[w * BM + r].y; }
            if (bm0 + r < M) ((float2*)e.stats_out)[(long)(bn0 / BN) * M + bm0 + r] = t;
        }
    }
#ifdef D2S_GLDS_TIMING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the epilogue's stores have left
    GL_STAMP(4)
#endif
}

// split-K second pass: sum the fp32 partials of all splits and run the fused epilogue once
template <typename T>
__global__ void __launch_bounds__(256)
splitk_reduce_kernel(GemmEpi e, int M, int N) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    int n4 = N >> 2;
    if (idx >= (long)M * n4) return;
    int m = (int)(idx / n4), n0 = (int)(idx % n4) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < e.ksplit; ++s) {
        float p[4];
        load4(e.part + ((long)s * M + m) * N + n0, p);
        v[0] += p[0]; v[1] += p[1]; v[2] += p[2]; v[3] += p[3];
    }
    epilogue_dispatch<T>(e, m, n0, v);
}

// ================================================================================================
// 3x3 convolution (stride 1, pad 1, NHWC) with the INPUT resident in LDS.  The implicit-GEMM loader above fetches
// every input pixel nine times from L2 (once per tap); here a block owns an 8 x 16 output tile, loads its 10 x 18 x C
// input halo ONCE (zero outside the image, ReLU-on-load applied at that point), and the K loop (9 taps x C) only
// streams the weights (LDS-DMA, two stages).  A fragment of tile row ty, tap (ky, kx) is halo pixel
// (ty + ky, fr + kx): 16 consecutive pixels per fragment, chunk index XOR-ed with the pixel index so the 16 lanes hit
// 16 different bank groups.  Same MFMA fragments, accumulators and epilogues as gemm_glds_kernel.
// Requirements (checked by the launcher): C * sizeof(T) a multiple of 128 (a K tile lies inside one tap), at most
// 16 chunks per pixel (C <= 128 bf16 / 64 f32), MAP_ROWS without row remapping, N >= 64.  Measured at batch 16:
// 84x148 RCU convs 118 -> 100 us (606 TFLOP/s), 42x74 45 -> 33 us, head conv1 271 -> 241 us.
// ================================================================================================
template <typename T, int BN, int WM, int WN, int NS = 2>
__global__ void __launch_bounds__(64 * WM * WN)
conv3_halo_kernel(GemmA a, const T* __restrict__ W, int M, int N, int K, int Kpad, GemmEpi e, int xn) {
    KERNARG_WARM(kaw_)                                   // all argument lines in one round trip (common.h)
    KERNARG_WARM_END(kaw_)
    constexpr int CE = Prec<T>::CE, CPR = 8, BK = CPR * CE, PD = NS - 1;
    constexpr int TW = 16, TH = 8, BM = TH * TW, HWD = TW + 2, HPX = (TH + 2) * HWD;
    constexpr int HCPP = 16;                            // capacity: 16-byte chunks per input pixel
    constexpr int NW = WM * WN, RPI = 64 / CPR;
    constexpr int BI = BN / (RPI * NW);
    static_assert(BI >= 1 && BM % (WM * 16) == 0 && BN % (WN * 16) == 0, "bad tile split");
    constexpr int FM = BM / WM / 16, FN = BN / WN / 16;
    constexpr int STAGE = BN * CPR;
    __shared__ __attribute__((aligned(16))) u32x4 lds[NS * STAGE + HPX * HCPP];
    D2S_POISON_LDS(lds, NS * STAGE + HPX * HCPP)
    u32x4* const halo = lds + NS * STAGE;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wid / WN, wave_n = wid % WN;
    const int tiles_x = (a.Wo + TW - 1) / TW, tiles_y = (a.Ho + TH - 1) / TH;
    const int nimg = M / (a.Ho * a.Wo);
    int tm_, tn_;
    if (!tile_of_block(blockIdx.x, nimg * tiles_y * tiles_x, (N + BN - 1) / BN, xn, tm_, tn_)) return;
    // (the tile origin inline, not conv3_tile.h's C3Tiles::org, as in conv3_halo2_kernel: with that prologue <f32,64,4,2,4> measured
    //  1-1.5 % slower -- profiles/conv3_shared_ab.md)
    const int b = tm_ / (tiles_y * tiles_x), ty0 = ((tm_ / tiles_x) % tiles_y) * TH, tx0 = (tm_ % tiles_x) * TW;
    const int bn0 = tn_ * BN;
    const int cpp = a.C / CE, smask = cpp - 1;          // chunks per pixel: a power of two <= 16

    // ---- weights: LDS-DMA ring, as in gemm_glds_kernel; the first NS - 1 K tiles are requested BEFORE the halo is fetched (they do not
    // depend on it: their latency sits under the halo phase -- with the up-sample folded in, four tap loads and the interpolation per chunk)
    const int lrow = wid * RPI + lane / CPR;
    const int src_chunk = (lane % CPR) ^ swz_row<CPR>(lrow);
    const T* wrow = W + (long)(bn0 + lrow) * Kpad + src_chunk * CE;
#define D2S_ISSUE_W(KT)                                                                                               \
    {                                                                                                                 \
        u32x4* st_ = lds + ((KT) % NS) * STAGE;                                                                       \
        _Pragma("unroll") for (int i = 0; i < BI; ++i)                                                                \
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wrow + (long)(RPI * NW * i) * Kpad + (KT) * BK), \
                                             (__attribute__((address_space(3))) void*)(st_ + (i * NW + wid) * 64), 16, 0, 0);              \
    }
    const int nkt = K / BK;
#pragma unroll
    for (int t = 0; t < PD; ++t)
        if (t < nkt) D2S_ISSUE_W(t)
    // ---- the input halo, once (a.ups: the align_corners up-sample in front of this convolution happens here; gemm_epi.h)
    conv_halo_fill<T, 64 * NW, 3>(a, b, ty0, tx0, HWD, HPX, cpp, tid, halo,
        [&](int p, int c) { return p * cpp + (c ^ (p & smask)); },
        [&](u32x4 v) { return a.relu ? relu_frag(v, 0, T()) : v; });
    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int kpt = cpp / CPR;                           // K tiles per tap
    const int fr = lane & 15, fg = lane >> 4;
    int tap = 0, sub = 0;                                // kt = tap * kpt + sub
    for (int kt = 0; kt < nkt; ++kt) {
        // my W loads of tile kt (tiles kt + 1 .. kt + PD - 1 may stay in flight) and, first time, my halo stores
        if (kt + PD - 1 < nkt) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((PD - 1) * BI) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (kt + PD < nkt) D2S_ISSUE_W(kt + PD)
        const int ky = tap / 3, kx = tap - ky * 3, cb = sub * CPR;
        const u32x4* B_l = lds + (kt % NS) * STAGE + (wave_n * (BN / WN)) * CPR;
#pragma unroll
        for (int ks = 0; ks < CPR / 4; ++ks) {
            u32x4 fb[FN];
#pragma unroll
            for (int j = 0; j < FN; ++j) { int r = j * 16 + fr; fb[j] = B_l[r * CPR + ((ks * 4 + fg) ^ swz_row<CPR>(r))]; }
#pragma unroll
            for (int i = 0; i < FM; ++i) {
                const int p = (wave_m * FM + i + ky) * HWD + fr + kx;
                const u32x4 fa = halo[p * cpp + ((cb + ks * 4 + fg) ^ (p & smask))];
#pragma unroll
                for (int j = 0; j < FN; ++j) mma_chunk(acc[i][j], fb[j], fa, T());
            }
        }
        if (++sub == kpt) { sub = 0; ++tap; }
    }
#undef D2S_ISSUE_W
    // ---- epilogue: tile row ty -> output pixel (ty0 + ty, tx0 + fr)
    const int nb = bn0 + wave_n * (BN / WN) + fg * 4;   // this lane's first column
    EpiCols cols[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j)
        if (nb + j * 16 < N) epi_cols_load(e, nb + j * 16, cols[j]);
    conv_tile_epilogue<T, FM, FN>(a, e, acc, cols, b, ty0 + wave_m * FM, tx0 + fr, nb, N);
}

// descriptor-addressed LDS-DMA: plain A, whole K tiles, 32-bit byte offsets
static inline bool buf_eligible(const GemmA& a, int M, int N, int K, int Kpad, int bk, size_t es) {
    return a.mode == A_PLAIN && !a.relu && K % bk == 0 && (long)M * a.lda * (long)es < (1L << 31) && (long)gemm_npad(N) * Kpad * (long)es < (1L << 31);
}

// split K below this many blocks (plan_glds)
constexpr int SPLITK_GRID = 128;

// would plan_glds split K for this launch (tiny grid, long K loop, caller-provided workspace)?  The lean instantiations take one K
// range per block (their ring is primed from preloaded arguments before e.ksplit could be read): lean_of sends such launches to the
// general instantiations.
static inline bool splitk_wanted(const GemmEpi& e, long tiles, int K, int bk) {
    return e.part && e.part_elems > 0 && !e.stats_out && tiles < SPLITK_GRID && cdiv(K, bk) >= 24;     // (splitk_reduce_kernel writes no LN statistics)
}

// deep-ring lean instantiations in the latency regime (lean_of); D2S_GEMM_DEEP=0: off
static bool gemm_deep() {
    static EnvInt deep{"D2S_GEMM_DEEP", 1};
    return deep.get() != 0;
}

// ---- the gemm_glds_kernel instantiations, one line each: X(id, operand types, BM,BN,WM,WN,NS,CPR,STG).  The kernel name, the
// geometry the planner reads and the launch all come from this list; an instantiation exists for the types its line names.
enum { TY_BF16 = 1, TY_E4M3 = 2, TY_F32 = 4, TY_BX3 = 8, TY_BEF = TY_BF16 | TY_E4M3 | TY_F32, TY_ALL = TY_BEF | TY_BX3 };
#define GLDS_INSTANCES(X)                                                                                                        \
    /* LDS-DMA ring (NS stages) */                                                                                               \
    X(G_256128, TY_BEF, 256,128,4,2,3,8,0)                                                                                       \
    X(G_128, TY_BEF, 128,128,2,2,4,8,0)                                                                                          \
    X(G_64, TY_BEF, 64,64,2,2,4,8,0)                                                                                             \
    /* (256-byte K tiles for this tile -- half the barrier-paced iterations -- measured at batch 1: 768 vs 766 frames/s with    \
        three ring stages, 726 with two: the batch-1 launches are not paced by their K-loop iteration count) */                  \
    X(G_3264, TY_ALL, 32,64,2,2,4,8,0)                                                                                           \
    /* (One-round shapes for M = 778 -- 48 x 64, 96 x 64, 48 / 96 / 80 / 112 x 128, 112 x 96: 108-240 blocks of 2-4 waves,     \
        fewer fill bytes per CU than two rounds of a small tile -- were instantiated and swept at batch 1: 1.2-4 x SLOWER than  \
        the 32 x 64 / 64 x 64 / 64 x 128 tiles on every encoder linear.  Resident waves per CU decide the fill rate a CU reaches.) \
       LDS-DMA, 8 waves, two stages: the winners of the second sweep (profiles/r1_05), code <BM><BN>8 */                         \
    X(G_1281288, TY_ALL, 128,128,2,4,2,8,0)    /* wave tile 64 x 32, 2 blocks / CU */                                            \
    X(G_641288, TY_ALL, 64,128,2,4,2,8,0)      /* 3 blocks / CU */                                                               \
    X(G_64648, TY_ALL, 64,64,4,2,2,8,0)        /* 5 blocks / CU */                                                               \
    X(G_256648, TY_BEF, 256,64,8,1,2,8,0)      /* WN == 1: MAP_HEAD capable */                                                   \
    X(G_128324, TY_BEF, 128,32,4,1,2,8,0)      /* WN == 1, 4 waves */                                                            \
    /* register-staged variants (STG), code = 9 <BM> <BN> [waves].  Removed after losing the sweeps: 256 x 128 / 256 x 256 with \
       8 waves (1 block / CU, lock-step), 128 x 128 with 4 or 16 waves, deeper rings, 64- and 256-byte K tiles, two register     \
       sets, intra-block split-K.  bf16x3 launches with an fp32 A run these only (the split happens on the way into LDS). */      \
    X(G_964, TY_ALL, 64,64,2,2,2,8,1)                                                                                            \
    X(G_91288, TY_ALL, 128,128,4,2,2,8,1)      /* 8 waves, 2 blocks / CU */                                                      \
    X(G_912832, TY_ALL, 128,32,4,1,2,8,1)      /* WN == 1: MAP_HEAD capable */                                                   \
    X(G_9256648, TY_ALL, 256,64,8,1,2,8,1)     /* WN == 1, 8 waves */                                                            \
    X(G_93264, TY_BX3, 32,64,2,2,2,8,1)                                                                                          \
    X(G_964128, TY_BX3, 64,128,2,4,2,8,1)                                                                                        \
    /* "lean" deep rings of the latency regime (lean_of): descriptor loader only */                                              \
    X(G_L3264, TY_BF16 | TY_E4M3 | TY_BX3, 32,64,2,2,6,8,2)      /* 72 KiB: 2 blocks / CU */                                    \
    X(G_L64648, TY_BF16 | TY_E4M3 | TY_BX3, 64,64,4,2,4,8,2)     /* 64 KiB: 2 blocks / CU */                                    \
    X(G_L641288, TY_BF16 | TY_E4M3 | TY_BX3, 64,128,2,4,3,8,2)   /* 72 KiB: 2 blocks / CU */

enum {
#define X(ID, ...) ID,
    GLDS_INSTANCES(X)
#undef X
};
struct GldsCfg { int types, BM, BN, WM, WN, NS, CPR, STG; };
static constexpr GldsCfg glds_cfg[] = {
#define X(ID, ...) {__VA_ARGS__},
    GLDS_INSTANCES(X)
#undef X
};
// [instantiation][operand type: bf16, e4m3, f32, bx3]
static const char* const glds_names[][4] = {
#define X(ID, TY, ...) {"gemm_glds_kernel<bf16," #__VA_ARGS__ ">", "gemm_glds_kernel<e4m3," #__VA_ARGS__ ">", \
                        "gemm_glds_kernel<f32," #__VA_ARGS__ ">", "gemm_glds_kernel<bx3," #__VA_ARGS__ ">"},
    GLDS_INSTANCES(X)
#undef X
};

// tile code -> instantiation, bf16 / e4m3 / fp32 operands (and a pre-split bf16x3 A, which the tile rule gives one of
// 3264 / 64648 / 641288 / 1281288)
static constexpr int glds_codes[][2] = {{256128, G_256128}, {128, G_128}, {64, G_64}, {3264, G_3264}, {1281288, G_1281288},
                                        {641288, G_641288}, {64648, G_64648}, {256648, G_256648}, {128324, G_128324}, {964, G_964},
                                        {91288, G_91288}, {912832, G_912832}, {9256648, G_9256648}};
// bf16x3 with an fp32 A: the register-staged tiles.  code (also reported), alias (the bf16 code of the same tile), the automatic
// rule's code this tile stands in for
static constexpr struct { int code, alias, auto_of, inst; } bx3_codes[] = {
    {93264, 3264, 3264, G_93264}, {964, 64, 64648, G_964}, {964128, 0, 641288, G_964128}, {91288, 128, 1281288, G_91288},
    {912832, 0, 912832, G_912832}, {9256648, 0, 9256648, G_9256648}};

// the conv3_halo_kernel instantiations: X(id, BN,WM,WN,NS), fp32 and bf16 operands.  (Ring depth: what keeps two blocks per CU beside
// the 46 KB halo -- four 8 KB stages for 64 output channels, two 16 KB stages for 128.)
#define HALO_INSTANCES(X) X(H_64, 64,4,2,4) X(H_128, 128,2,4,2)
enum {
#define X(ID, ...) ID,
    HALO_INSTANCES(X)
#undef X
};
static constexpr struct { int BN, WM, WN, NS; } halo_cfg[] = {
#define X(ID, ...) {__VA_ARGS__},
    HALO_INSTANCES(X)
#undef X
};
static const char* const halo_names[][4] = {
#define X(ID, ...) {"conv3_halo_kernel<bf16," #__VA_ARGS__ ">", nullptr, "conv3_halo_kernel<f32," #__VA_ARGS__ ">", nullptr},
    HALO_INSTANCES(X)
#undef X
};

// column of the name tables: the operand type of a GEMM precision (anything else runs as fp32, like elem_size)
static inline int type_index(int precision) {
    return precision == D2S_PREC_BF16 ? 0 : (precision == D2S_PREC_FP8_OPERANDS ? 1 : (precision == D2S_PREC_BF16X3 ? 3 : 2));
}
template <typename T> constexpr int type_bit() {
    return std::is_same<T, bf16_t>::value ? TY_BF16 : std::is_same<T, fp8_t>::value ? TY_E4M3 : std::is_same<T, bx3_t>::value ? TY_BX3 : TY_F32;
}

static int plan_fail(GemmPlan& p, int rc, const char* msg) { p.error = msg; return rc; }
static int glds_inst_of(int code) {
    for (const auto& c : glds_codes) if (c[0] == code) return c[1];
    return -1;
}

// gemm_glds_kernel instantiation inst, reported as tile code `tile`: XCD grid, split-K, descriptor addressing, statistics slots
static int plan_glds(int inst, int precision, int tile, const GemmA& a, int M, int N, int K, int Kpad, const GemmEpi& e, GemmPlan& p) {
    const GldsCfg& c = glds_cfg[inst];
    const int es = (int)elem_size(precision), bk = c.CPR * (16 / es);
    p.family = GEMM_GLDS; p.inst = inst; p.name = glds_names[inst][type_index(precision)]; p.tile = tile; p.block = 64 * c.WM * c.WN;
    p.xn = pick_xn(cdiv(M, c.BM), cdiv(N, c.BN), c.BN, Kpad, es, p.grid);
    // split-K for the few launches with almost no tiles but a long K loop (DPT 3x3 convs on the 11x19 /
    // 21x37 maps with 768 input channels: 14-112 blocks x 108 K tiles): the caller provides e.part
    const int nkt = cdiv(K, bk);
    int ks = 1;
    if (c.STG != 2 && e.part && e.part_elems > 0 && !e.stats_out && (int)p.grid < SPLITK_GRID && nkt >= 24) {
        ks = nkt / 6; if (ks > 16) ks = 16;
        while (ks > 1 && (size_t)ks * M * N > e.part_elems) --ks;
    }
    static EnvInt sk_force{"D2S_SPLITK_FORCE", 0};          // measurement aid (tools/splitk_probe.py): this many K ranges whatever the grid
    if (sk_force.get() > 1 && c.STG != 2 && e.part && !e.stats_out && nkt >= sk_force.get() && (size_t)sk_force.get() * M * N <= e.part_elems) ks = sk_force.get();
    p.ksplit = ks; p.gridy = ks;
    if (ks > 1) { p.grid2 = cdiv((long)M * (N / 4), 256); return D2S_OK; }      // partials, then splitk_reduce_kernel
    p.stats_slots = c.WN > 1 ? cdiv(N, c.BN) : 1 << 20;        // WN == 1 tiles write no statistics: the caller falls back
    // descriptor-addressed LDS-DMA: plain A, whole K tiles (the W zero padding covers nothing then), 32-bit byte offsets
    p.buf = c.STG != 1 && buf_eligible(a, M, N, K, Kpad, bk, es);
    return D2S_OK;
}

// Latency regime (batch 1-2: every block of the launch is resident at once, 1-2 per CU).  In-kernel stamps (tools/glds_timeline.py)
// put a K tile at (LDS-DMA latency ~ 1 800 cycles) / (tiles in flight): 615 cycles with the 4-stage ring of the 32 x 64 tile, 1 100-1 300
// with the 2-stage rings of the 8-wave tiles, next to 64-256 cycles of MFMA work.  The LDS those few blocks leave unused buys
// ring depth: as many stages as still let ALL blocks be resident.  The "lean" instantiation for tile code t (descriptor loader only),
// or -1.
// (one block per CU with a 128 KiB ring -- 64 x 192 x 4 stages, 128 x 128 on 64-byte K tiles x 4 stages -- for FC1, whose 312
//  blocks of 64 x 128 leave 56 CUs with two blocks: 13.5 / 15.6 us against 13.4 back to back; a single block does not reach
//  the fill rate two reach together.  Measured, removed.)
// (The same deeper rings for the implicit 3x3 convolutions of the small DPT maps at batch 1 -- general loaders, 32 x 64 x 6 / 64 x 64 x 4 /
//  64 x 128 x 3 stages when every block is resident: 866-873 frames/s with and without, ViT-S 1 200 vs 1 227.  Measured, removed.)
static int lean_of(int t, int precision, const GemmA& a, int M, int N, int K, int Kpad, const GemmEpi& e) {
    const int inst = t == 3264 ? G_L3264 : (t == 64648 ? G_L64648 : (t == 641288 ? G_L641288 : -1));
    if (inst < 0 || !gemm_deep() || !buf_eligible(a, M, N, K, Kpad, gemm_bk(precision), elem_size(precision))) return -1;
    const long tiles = (long)cdiv(M, glds_cfg[inst].BM) * cdiv(N, glds_cfg[inst].BN);
    return tiles <= 512 && !splitk_wanted(e, tiles, K, gemm_bk(precision)) ? inst : -1;
}

// the tile code of a plain linear of this shape, N > 64: 1281288, 641288, 64648, or 3264 for the skinny launches (batch 1, N = 768)
static int small_tile_of(int M, int N) {
    const long b128 = (long)cdiv(M, 128) * cdiv(N, 128), b64128 = (long)cdiv(M, 64) * cdiv(N, 128), b64 = (long)cdiv(M, 64) * cdiv(N, 64);
    if (b128 >= 400 && (N >= 1536 || b128 >= 900)) return 1281288;
    if (b64128 >= 280) return 641288;
    if (b64 >= 384) return 64648;
    return 3264;
}

// The automatic tile rule (tile == 0).  Measured on the ViT-B shapes at batch 1..32 (tools/gemm_bench.py, profiles/r1_05): what matters
// most is 16-24 resident waves per CU in DIFFERENT phases of the K loop (8-wave blocks, 2-5 blocks per CU), then tile intensity; with
// that in place the LDS-DMA path beats register staging (no VGPR / ds_write pass).  The 4-wave 32 x 64 ring (NS = 4: deepest prefetch,
// shortest prologue) keeps the launches with the fewest tiles (batch 1: proj, FC2).
static int auto_tile(int M, int N) {
    if (N <= 64) return (long)cdiv(M, 256) >= 224 ? (N <= 32 ? 912832 : 9256648) : 3264;      // DPT head: 64 / 32 output channels, M = pixels
    return small_tile_of(M, N);
}

// stride-1 3x3 convs on the large maps go to conv3_halo_kernel (input tile resident in LDS); D2S_NO_HALO=1 keeps the
// implicit-GEMM loader (the parity tests run both)
static bool plan_halo(int precision, const GemmA& a, int M, int N, int K, int Kpad, const GemmEpi& e, GemmPlan& p) {
    static EnvInt off{"D2S_NO_HALO", 0};
    if (off.get() || precision == D2S_PREC_FP8_OPERANDS) return false;
    const int es = (int)elem_size(precision), cpp = a.C * es / 16;
    if (a.mode != A_CONV3 || a.stride != 1 || a.Hi != a.Ho || a.Wi != a.Wo || (a.C * es) % 128 || cpp > 16 || (cpp & (cpp - 1))) return false;
    if (e.map != MAP_ROWS || e.rows_per_img || K != 9 * a.C || N <= 32) return false;   // (the N = 32 head conv measured 20 % slower here)
    const int nimg = M / (a.Ho * a.Wo);
    const long tiles_m = (long)nimg * cdiv(a.Ho, 8) * cdiv(a.Wo, 16);
    if (tiles_m * cdiv(N, 128) < 200 || (long)nimg * a.Ho * a.Wo != M) return false;      // small maps: too few tiles, latency-bound anyway
    const int inst = N <= 64 ? H_64 : H_128, bn = halo_cfg[inst].BN;
    p.family = GEMM_HALO; p.inst = inst; p.block = 64 * halo_cfg[inst].WM * halo_cfg[inst].WN; p.ups = a.ups;
    p.name = halo_names[inst][type_index(precision)];
    p.xn = pick_xn((int)tiles_m, cdiv(N, bn), bn, Kpad, es, p.grid);
    return true;
}

// (Weight warm-up, measured and removed: a small kernel on its own stream pulling the NEXT linear's weight rows into the L2 of the
//  XCDs that will read them, two launches ahead -- 761-778 frames/s at batch 1 with and without.  Like the K-loop instruction
//  count (descriptor addressing: +2 %), the K-tile size (256-byte tiles: +-0) and split-K for FC2 (-5 %), cold weights are not
//  what paces the batch-1 launches.)
int gemm_pp_min_tiles() {
    static EnvInt v{"D2S_GEMM_PP", 100};                  // (re-read after d2s_debug_reload_env: the tests switch regimes inside one process)
    return v.get();
}

// Everything launch_gemm does, decided from the arguments, the D2S_* switches and the CU count.  Host only: no launch, allocation or
// stream work, so conv3_upsample_ok can ask it too.  On a rejected input p.error says why.
int plan_gemm(int precision, int tile, const GemmA& a, int M, int N, int K, int Kpad, const GemmEpi& e, GemmPlan& p) {
    p = GemmPlan{};
    p.gridy = 1; p.ksplit = 1; p.buf = a.buf; p.stats_slots = -1;
    const int ce = 16 / (int)elem_size(precision);
    if (M <= 0 || N <= 0 || K <= 0 || (N & 3) || (K % ce) || Kpad % (2 * gemm_bk(precision)))
        return plan_fail(p, D2S_E_INVALID, "launch_gemm: bad dims (N % 4, K % chunk, Kpad % BK)");
    if (a.mode == A_PLAIN && (a.lda % ce)) return plan_fail(p, D2S_E_INVALID, "launch_gemm: lda not chunk aligned");
    if (a.mode == A_CONV3 && (a.C % ce)) return plan_fail(p, D2S_E_INVALID, "launch_gemm: conv channels not chunk aligned");
    if (precision == D2S_PREC_BF16X3) {
        if (e.deq || (e.out2 && !e.out2_bx3))
            return plan_fail(p, D2S_E_UNSUPPORTED, "launch_gemm: bf16x3 operands: no de-quantisation, raw-residual copies in the unit format only");
        if (a.bx3) {
            // A pre-split by its producer (LayerNorm / attention / GELU epilogue): LDS-DMA rings for both operands, the bf16 tile rule
            // and, in the latency regime, its lean rings
            if (a.mode != A_PLAIN || a.relu) return plan_fail(p, D2S_E_UNSUPPORTED, "launch_gemm: a pre-split bf16x3 A operand must be a plain matrix");
            const int t = small_tile_of(M, N), lean = lean_of(t, precision, a, M, N, K, Kpad, e);
            return plan_glds(lean >= 0 ? lean : glds_inst_of(t), precision, t, a, M, N, K, Kpad, e, p);
        }
        // fp32 A: the register-staged tiles only (the fp32 -> hi / lo split happens between the staging registers and LDS), picked by
        // the same rule as the other types -- resident waves first, then tile intensity
        if (tile == 256256) tile = 0;           // (the ping-pong tile code names no bf16x3 kernel: the automatic rule)
        const int t = tile ? tile : auto_tile(M, N);
        for (const auto& c : bx3_codes)
            if (tile ? (tile == c.code || tile == c.alias) : t == c.auto_of) return plan_glds(c.inst, precision, tile ? tile : c.code, a, M, N, K, Kpad, e, p);
        return plan_fail(p, D2S_E_INVALID, "launch_gemm: bad tile code for bf16x3 operands");
    }
    if (tile == 256256) return plan_gemm_pp(precision, a, M, N, K, Kpad, e, p);      // the ping-pong kernel, forced (tests / sweeps)
    // batched 3x3 convolutions (and the fused head, whose caller names a tile): input tile resident in LDS, conv3.hip
    if (precision == D2S_PREC_BF16 && a.mode == A_CONV3 && (tile == 0 || e.map == MAP_HEAD) && plan_conv3_halo2(a, M, N, K, Kpad, e, p)) return D2S_OK;
    if (a.ups) {        // only the LDS-resident-input kernels fold the up-sample (conv3_upsample_ok says when)
        if (precision == D2S_PREC_BF16 && tile == 0 && plan_halo(precision, a, M, N, K, Kpad, e, p)) return D2S_OK;
        return plan_fail(p, D2S_E_UNSUPPORTED, "launch_gemm: this launch cannot fold the up-sample into its loader (conv3_upsample_ok says when)");
    }
    if (precision == D2S_PREC_FP8_OPERANDS && (a.mode != A_PLAIN || a.relu)) return plan_fail(p, D2S_E_UNSUPPORTED, "launch_gemm: e4m3 operands are for plain linears");
    if (tile == 0 && plan_halo(precision, a, M, N, K, Kpad, e, p)) return D2S_OK;
    // thin linears (K <= 256: ConvTranspose(k = s), fusion 1x1 projections): HBM-bound, one prologue per block instead of per tile
    if (tile == 0 && sk_supported(precision, a, M, N, K, Kpad, e)) { plan_gemm_sk(a, M, N, K, p); return D2S_OK; }
    // batched plain linears: the 256 x 256 ping-pong kernel (gemm_pp.hip) once the launch has enough tiles to fill the chip (bf16 and
    // e4m3 operands: pp_supported).  Measured (tools/pp_check.py, ViT-B shapes): from ~140 tiles of 256 x 256 the ping-pong kernel wins
    // every encoder linear (batch 16: +14..+30 %, batch 32: +9..+48 %); at 75 tiles (batch 8, N = 768) it loses.  D2S_GEMM_PP=0: off
    // (100 vs 140: +5 % at batch 12, proj / FC2 there)
    // (Tile rounding, batch 32: 294 tiles of N = 768 pay a second round for 38 tiles.  Giving the ping-pong kernel only the
    //  tile rows that fill whole rounds and the remaining 3136 rows to the small-tile kernel -- two launches, disjoint rows --
    //  was built and measured: FC2 156 -> 148 us, proj unchanged; the small-tile kernel needs as long for those rows as the
    //  half-empty round.  Removed.)
    const int pp_min_tiles = gemm_pp_min_tiles();
    if (tile == 0 && pp_min_tiles > 0 && (long)cdiv(M, 256) * cdiv(N, 256) >= pp_min_tiles && pp_supported(precision, a, M, N, K, Kpad, e))
        return plan_gemm_pp(precision, a, M, N, K, Kpad, e, p);
    if (tile == 0) {
        tile = auto_tile(M, N);
        // long-K implicit convolutions (tap 3's stride-2 768 -> 768: K = 6 912) from ~300 tiles of 128 x 128: the 64 x 128 tile falls off a
        // cliff there (batch 28: 130 us, batch 32: 188 us for 1.14 x the work) where the 128 x 128 tile stays at 128-134 us at every batch from
        // 16 to 32 -- below 300 tiles the smaller tile is 5-15 % faster
        if (N > 64 && a.mode == A_CONV3 && K >= 4096 && (long)cdiv(M, 128) * cdiv(N, 128) >= 300) tile = 1281288;
    }
    // the lean rings (bf16 and e4m3 operands) keep to launches without a MAP_HEAD epilogue or a caller-chosen K split
    if ((precision == D2S_PREC_BF16 || precision == D2S_PREC_FP8_OPERANDS) && !(e.part && e.ksplit > 1) && e.map != MAP_HEAD) {
        const int lean = lean_of(tile, precision, a, M, N, K, Kpad, e);
        if (lean >= 0) return plan_glds(lean, precision, tile, a, M, N, K, Kpad, e, p);
    }
    const int inst = glds_inst_of(tile);
    if (inst < 0) return plan_fail(p, D2S_E_INVALID, "launch_gemm: bad tile code");
    return plan_glds(inst, precision, tile, a, M, N, K, Kpad, e, p);
}

// Would launch_gemm fold the up-sample described by a.ups / Hs / Ws / usy / usx into this convolution's loader?  (The engine asks
// before it skips the stand-alone up-sample launch.)
bool conv3_upsample_ok(int precision, int tile, const GemmA& a, int M, int N, int K, int Kpad, const GemmEpi& e) {
    static EnvInt no_ups{"D2S_NO_UPSFOLD", 0};
    if (no_ups.get() || precision != D2S_PREC_BF16 || a.mode != A_CONV3 || !a.ups || a.Hs < 2 || a.Ws < 2 || a.usy <= 0.f || a.usx <= 0.f) return false;
    GemmPlan p;
    return plan_gemm(precision, tile, a, M, N, K, Kpad, e, p) == D2S_OK && p.ups;
}

// the planned gemm_glds_kernel / conv3_halo_kernel instantiation for operand type T (and the split-K reduce)
template <typename T>
static void launch_glds(const GemmPlan& p, const GemmA& a, const void* W, int M, int N, int K, int Kpad, const GemmEpi& e, hipStream_t st,
                        hipEvent_t stop) {
    const dim3 grid(p.grid, p.gridy), block(p.block);
    const hipEvent_t stop1 = p.grid2 ? nullptr : stop;      // (split-K: the reduce is the launch's last kernel)
    if (p.family == GEMM_HALO) {
        if constexpr ((type_bit<T>() & (TY_BF16 | TY_F32)) != 0) switch (p.inst) {
#define X(ID, ...) case ID: hipLaunchKernelGGL((conv3_halo_kernel<T, __VA_ARGS__>), grid, block, 0, st, a, (const T*)W, M, N, K, Kpad, e, p.xn); break;
            HALO_INSTANCES(X)
#undef X
        }
        return;
    }
    switch (p.inst) {
#define X(ID, TY, ...) case ID: if constexpr (((TY) & type_bit<T>()) != 0) \
        D2S_LAUNCH_STOP(stop1, (gemm_glds_kernel<T, __VA_ARGS__>), grid, block, st, (const T*)W, a.ptr, a.lda, M, N, K, Kpad, p.xn, a, e); break;
        GLDS_INSTANCES(X)
#undef X
    }
    if (p.grid2) D2S_LAUNCH_STOP(stop, (splitk_reduce_kernel<T>), dim3(p.grid2), dim3(256), st, e, M, N);
}

static void note_kernel(const GemmPlan& p) { kernel_note() = KernelNote{p.name, p.tile, p.ksplit, p.tail}; }

int launch_gemm(int precision, int tile, const GemmA& a, const void* W, int M, int N, int K, int Kpad,
                const GemmEpi& e, hipStream_t st, hipEvent_t stop) {
    GemmPlan p;
    if (const int rc = plan_gemm(precision, tile, a, M, N, K, Kpad, e, p)) { set_error(p.error); return rc; }
    note_kernel(p);
    const bool in_launch = p.family == GEMM_GLDS || p.family == GEMM_PP;     // the families that take `stop` with their dispatch
    if (e.stats_slots && p.stats_slots >= 0) *e.stats_slots = p.stats_slots;
    GemmA a1 = a;
    a1.buf = p.buf;
    GemmEpi e1 = e;
    e1.ksplit = p.family == GEMM_GLDS ? p.ksplit : 1;
    switch (p.family) {
        case GEMM_CONV3: launch_conv3_halo2(p, a1, W, M, N, Kpad, e1, st); break;
        case GEMM_SK: launch_gemm_sk(p, a1, W, M, N, Kpad, e1, st); break;
        case GEMM_PP: if (const int rc = launch_gemm_pp(p, precision, a1, W, M, N, K, Kpad, e1, st, stop)) return rc; break;
        default: {
            const hipEvent_t ev = in_launch ? stop : nullptr;                  // (GEMM_HALO shares this launcher: recorded below)
            if (precision == D2S_PREC_BF16) launch_glds<bf16_t>(p, a1, W, M, N, K, Kpad, e1, st, ev);
            else if (precision == D2S_PREC_FP8_OPERANDS) launch_glds<fp8_t>(p, a1, W, M, N, K, Kpad, e1, st, ev);
            else if (precision == D2S_PREC_BF16X3) launch_glds<bx3_t>(p, a1, W, M, N, K, Kpad, e1, st, ev);
            else launch_glds<float>(p, a1, W, M, N, K, Kpad, e1, st, ev);
        }
    }
    D2S_CHECK_LAUNCH();
    if (stop && !in_launch) D2S_HIP(hipEventRecord(stop, st));
    return D2S_OK;
}

// ---- test / micro-benchmark probe -----------------------------------------------------------------
__global__ void cast_pad_kernel(const float* __restrict__ src, void* __restrict__ dst, int rows, int cols,
                                int rows_pad, int cols_pad, int prec) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)rows_pad * cols_pad) return;
    int c = (int)(idx % cols_pad), r = (int)(idx / cols_pad);
    float v = (r < rows && c < cols) ? src[(long)r * cols + c] : 0.f;
    if (prec == -D2S_PREC_BF16X3) {                  // a bf16x3 WEIGHT matrix: unit format (the A operand stays fp32: prec == D2S_PREC_BF16X3 below)
        const bf16_t hi = f2bf(v), lo = f2bf(v - bf2f(hi));
        bf16_t* u = (bf16_t*)((char*)dst + ((long)r * cols_pad + (c & ~7)) * 4) + (c & 7);
        u[0] = hi; u[8] = lo;
    } else
    if (prec == D2S_PREC_BF16) ((bf16_t*)dst)[idx] = f2bf(v);
    else if (prec == D2S_PREC_FP8_OPERANDS) ((fp8_t*)dst)[idx] = f2e4m3(v);      // unit scales: the caller keeps |v| <= 448
    else ((float*)dst)[idx] = v;
}

}  // namespace d2s

using namespace d2s;

// ---- probes: host-side helpers -----------------------------------------------------------------
namespace d2s {

static thread_local KernelNote g_kernel_note = {};
KernelNote& kernel_note() { return g_kernel_note; }

namespace {
struct ProbeBuf {                    // device scratch of a probe, freed on every return path
    void* p = nullptr;
    ProbeBuf() = default;
    ProbeBuf(const ProbeBuf&) = delete;
    ProbeBuf& operator=(const ProbeBuf&) = delete;
    ~ProbeBuf() { if (p) (void)hipFree(p); }
};

// host copy of a device float matrix
int fetch_f32(std::vector<float>& h, const float* d, size_t n) {
    h.resize(n);
    D2S_HIP(hipMemcpy(h.data(), d, n * sizeof(float), hipMemcpyDeviceToHost));
    return D2S_OK;
}
int upload(ProbeBuf& buf, const void* h, size_t bytes) {
    D2S_HIP(hipMalloc(&buf.p, bytes));
    D2S_HIP(hipMemcpy(buf.p, h, bytes, hipMemcpyHostToDevice));
    return D2S_OK;
}

// a split-K workspace as the engine holds one (engine.hip splitk_ws): elems fp32 partials followed by GEMM_PART_CTR_WORDS counter
// words, zeroed in stream order -- the words behind the partials must be zero when a launch reads them (gemm.h)
int alloc_splitk_ws(ProbeBuf& buf, size_t elems, hipStream_t st) {
    const size_t bytes = (elems + GEMM_PART_CTR_WORDS) * sizeof(float);
    D2S_HIP(hipMalloc(&buf.p, bytes));
    D2S_HIP(hipMemsetAsync(buf.p, 0, bytes, st));
    return D2S_OK;
}

// the kernel the last launch recorded (kernel_note), as the probes report it: gemm_glds_kernel with its tile code and split-K ranges,
// the ping-pong kernel with its tail units and how they are finished
std::string noted_kernel() {
    const KernelNote kn = kernel_note();
    std::string name = kn.name ? kn.name : "unrecorded";
    if (kn.name && !strncmp(kn.name, "gemm_glds_kernel", 16)) {
        name += " tile=" + std::to_string(kn.tile);
        if (kn.ksplit > 1) name += " splitk=" + std::to_string(kn.ksplit);
    } else if (kn.name && kn.tail != NOTE_TAIL_NONE) {
        static const char* const tails[4] = {"", "in-kernel", "two-launch", "row-split"};
        name += " ks=" + std::to_string(kn.ksplit) + " tail=" + tails[kn.tail];
    }
    return name;
}
}  // namespace

}  // namespace d2s

extern "C" int d2s_gemm_probe(const float* A, const float* Wt, const float* bias, float* Cout, int M, int N, int K,
                              int precision, int tile, int iters, void* stream) {
    D2S_REQUIRE(A && Wt && Cout && M > 0 && N > 0 && K > 0 && (N % 4 == 0) && iters >= 1, "bad argument");
    D2S_REQUIRE(precision == D2S_PREC_BF16 || precision == D2S_PREC_FP32 || precision == D2S_PREC_FP8_OPERANDS || precision == D2S_PREC_BF16X3, "bad precision");
    hipStream_t st = (hipStream_t)stream;
    int bf = precision;
    int Kp = gemm_kpad(K, precision), Np = gemm_npad(N);
    size_t es = elem_size(precision);
    ProbeBuf dA, dW, dP;
    D2S_HIP(hipMalloc(&dA.p, (size_t)M * Kp * es));
    D2S_HIP(hipMalloc(&dW.p, (size_t)Np * Kp * es));
    hipLaunchKernelGGL(cast_pad_kernel, dim3(cdiv((long)M * Kp, 256)), dim3(256), 0, st, A, dA.p, M, K, M, Kp, bf);
    hipLaunchKernelGGL(cast_pad_kernel, dim3(cdiv((long)Np * Kp, 256)), dim3(256), 0, st, Wt, dW.p, N, K, Np, Kp, bf == D2S_PREC_BF16X3 ? -bf : bf);
    GemmA a = {};
    a.ptr = dA.p; a.mode = A_PLAIN; a.lda = Kp;
    GemmEpi e = {};
    e.out = Cout; e.out_type = OUT_F32; e.ldc = N; e.bias = bias;
    static EnvInt sk_force{"D2S_SPLITK_FORCE", 0};          // measurement aid: give the launch a split-K workspace
    if (sk_force.get() > 1) {
        const size_t pe = (size_t)sk_force.get() * M * N;
        int rc = alloc_splitk_ws(dP, pe, st);
        if (rc != D2S_OK) return rc;
        e.part = (float*)dP.p; e.part_elems = pe;
    }
    int rc = D2S_OK;
    for (int i = 0; i < iters && rc == D2S_OK; ++i) rc = launch_gemm(precision, tile, a, dW.p, M, N, Kp, Kp, e, st);
    hipError_t err = hipStreamSynchronize(st);
    if (rc != D2S_OK) return rc;
    D2S_HIP(err);
    return D2S_OK;
}

extern "C" int d2s_conv3_probe(d2s_conv3_probe_params* p, void* stream) {
    D2S_REQUIRE(p && p->struct_size == sizeof(d2s_conv3_probe_params), "d2s_conv3_probe_params.struct_size must be sizeof(d2s_conv3_probe_params)");
    p->kernel[0] = 0;
    const int prec = p->precision, B = p->batch, C = p->C, N = p->N;
    D2S_REQUIRE(prec == D2S_PREC_BF16 || prec == D2S_PREC_FP32 || prec == D2S_PREC_BF16X3, "bad precision (bf16, fp32 or bf16x3)");
    D2S_REQUIRE(p->x && p->w && p->out && B > 0 && C > 0 && N > 0 && p->Hs > 0 && p->Ws > 0 && p->Hi > 0 && p->Wi > 0, "bad argument");
    D2S_REQUIRE(p->stride == 1 || p->stride == 2, "stride must be 1 or 2");
    const bool ups = p->Hs != p->Hi || p->Ws != p->Wi;
    D2S_REQUIRE(!ups || p->stride == 1, "a folded up-sample needs stride 1");
    D2S_REQUIRE(!p->map_head || (p->w3 && !p->res && p->act == 0 && p->stride == 1), "map_head: w3 needed; no residual, no act, stride 1");
    hipStream_t st = (hipStream_t)stream;
    const int Ho = (p->Hi + 2 - 3) / p->stride + 1, Wo = (p->Wi + 2 - 3) / p->stride + 1;
    const long M = (long)B * Ho * Wo, nsrc = (long)B * p->Hs * p->Ws;
    D2S_REQUIRE(M < (1L << 31) && nsrc * C < (1L << 31), "too large");
    const int K = 9 * C, Kp = gemm_kpad(K, prec);
    const bool bf = prec == D2S_PREC_BF16;             // bf16 engine: bf16 activations; fp32 / bf16x3 engines: fp32 activations
    const bool out_t = !p->out_f32 && !p->map_head;    // OUT_T: bf16 on the bf16 engine, fp32 otherwise
    ProbeBuf dW, dX, dR, dP;
    {   // the weight packed as pack_conv3 packs it
        std::vector<float> w;
        int rc = fetch_f32(w, p->w, (size_t)N * C * 9);
        if (rc == D2S_OK) {
            const LinearImage im = prepare_linear(prec, N, K, [&](int n, int k) { return w[conv3_weight_index(n, k, C)]; }, nullptr);
            rc = upload(dW, im.w.data(), im.w.size());
        }
        if (rc != D2S_OK) return rc;
    }
    const void* x = p->x;
    if (bf) {
        D2S_HIP(hipMalloc(&dX.p, (size_t)nsrc * C * 2));
        hipLaunchKernelGGL(cast_pad_kernel, dim3(cdiv(nsrc * C, 256)), dim3(256), 0, st, p->x, dX.p, (int)nsrc, C, (int)nsrc, C, D2S_PREC_BF16);
        x = dX.p;
    }
    const void* res = p->res;                         // residual: the output's type
    if (res && bf && out_t) {
        D2S_HIP(hipMalloc(&dR.p, (size_t)M * N * 2));
        hipLaunchKernelGGL(cast_pad_kernel, dim3(cdiv(M * N, 256)), dim3(256), 0, st, p->res, dR.p, (int)M, N, (int)M, N, D2S_PREC_BF16);
        res = dR.p;
    }
    D2S_HIP(hipExtGetLastError());
    // GemmA / GemmEpi as engine.hip builds them: convA() + conv3()'s rowsE for a convolution, the head's MAP_HEAD tail for conv2,
    // the up-sample fields of the head's conv1 / conv2 launches
    GemmA a = {};
    a.ptr = x; a.mode = A_CONV3; a.Hi = p->Hi; a.Wi = p->Wi; a.C = C; a.Ho = Ho; a.Wo = Wo; a.stride = p->stride; a.relu = p->relu_in;
    if (ups) { a.ups = 1; a.Hs = p->Hs; a.Ws = p->Ws; a.usy = linear_scale(p->Hs, p->Hi, true); a.usx = linear_scale(p->Ws, p->Wi, true); }
    GemmEpi e = {};
    e.out = p->out; e.out_type = out_t ? OUT_T : OUT_F32; e.ldc = N; e.bias = p->bias;
    e.act = p->act ? ACT_RELU : ACT_NONE; e.res1 = res;
    if (p->map_head) { e.ldc = 1; e.map = MAP_HEAD; e.scale = p->w3; e.head_b3 = p->b3; e.head_max_depth = p->max_depth; }
    const int tile = p->tile ? p->tile : (p->map_head ? head_tile(N <= 32 ? 32 : 64) : 0);
    if (p->splitk_elems > 0) {
        int rc = alloc_splitk_ws(dP, (size_t)p->splitk_elems, st);
        if (rc != D2S_OK) return rc;
        e.part = (float*)dP.p; e.part_elems = (size_t)p->splitk_elems;
    }
    if (ups && !conv3_upsample_ok(prec, tile, a, (int)M, N, K, Kp, e)) {
        set_error("d2s_conv3_probe: conv3_upsample_ok refuses to fold this up-sample");
        return D2S_E_UNSUPPORTED;
    }
    kernel_note() = KernelNote{nullptr, 0, 1};
    int rc = launch_gemm(prec, tile, a, dW.p, (int)M, N, K, Kp, e, st);
    hipError_t err = hipStreamSynchronize(st);
    if (rc != D2S_OK) return rc;
    D2S_HIP(err);
    snprintf(p->kernel, sizeof(p->kernel), "%s", noted_kernel().c_str());
    return D2S_OK;
}

// ---- d2s_rcu_probe ------------------------------------------------------------------------------------------------------
extern "C" int d2s_rcu_probe(d2s_rcu_probe_params* p, void* stream) {
    D2S_REQUIRE(p && p->struct_size == sizeof(d2s_rcu_probe_params), "d2s_rcu_probe_params.struct_size must be sizeof(d2s_rcu_probe_params)");
    p->kernel[0] = 0;
    const int B = p->batch, H = p->H, W = p->W, C = p->C;
    D2S_REQUIRE(p->x && p->w1 && p->b1 && p->w2 && p->b2 && p->out && B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "bad argument");
    D2S_REQUIRE(!p->wp == !p->bp, "the projection needs its weight and its bias");
    hipStream_t st = (hipStream_t)stream;
    const long npx = (long)B * H * W;
    D2S_REQUIRE(npx * C < (1L << 31), "too large");
    GemmPlan plan;
    D2S_REQUIRE(p->reserved == 0 || p->reserved == 1, "reserved selects the tile form: 0 or 1");
    if (!plan_conv3_rcu(true, C, B, H, W, p->wp != nullptr, p->reserved == 1, plan)) {
        set_error(p->reserved ? "d2s_rcu_probe: c3_rcu_wide_fits refuses this map (C = 128 and 8 x 8-pixel tiles x images <= CU count)"
                              : "d2s_rcu_probe: c3_rcu_ok refuses this map (C = 128 and tiles x images <= CU count)");
        return D2S_E_UNSUPPORTED;
    }
    // the weights packed as pack_conv3 / pack_linear pack them
    ProbeBuf dW[3], dX;
    int Kpad[3] = {0, 0, 0};
    for (int i = 0; i < 3; ++i) {
        const float* src = i == 0 ? p->w1 : (i == 1 ? p->w2 : p->wp);
        if (!src) continue;
        const int K = i < 2 ? 9 * C : C;
        std::vector<float> w;
        int rc = fetch_f32(w, src, (size_t)C * K);
        if (rc != D2S_OK) return rc;
        const LinearImage im = i < 2 ? prepare_linear(D2S_PREC_BF16, C, K, [&](int n, int k) { return w[conv3_weight_index(n, k, C)]; }, nullptr)
                                     : prepare_linear(D2S_PREC_BF16, C, K, [&](int n, int k) { return w[(size_t)n * K + k]; }, nullptr);
        rc = upload(dW[i], im.w.data(), im.w.size());
        if (rc != D2S_OK) return rc;
        Kpad[i] = im.Kpad;
    }
    D2S_HIP(hipMalloc(&dX.p, (size_t)npx * C * 2));
    hipLaunchKernelGGL(cast_pad_kernel, dim3(cdiv(npx * C, 256)), dim3(256), 0, st, p->x, dX.p, (int)npx, C, (int)npx, C, D2S_PREC_BF16);
    D2S_HIP(hipExtGetLastError());
    const RcuOp o = {dX.p, p->out, B, H, W, dW[0].p, dW[1].p, dW[2].p, p->b1, p->b2, p->bp, Kpad[0], Kpad[2]};
    kernel_note() = KernelNote{nullptr, 0, 1, NOTE_TAIL_NONE};
    launch_conv3_rcu(plan, o, st);
    D2S_HIP(hipStreamSynchronize(st));
    snprintf(p->kernel, sizeof(p->kernel), "%s", noted_kernel().c_str());
    return D2S_OK;
}

// ---- d2s_linear_probe ---------------------------------------------------------------------------------------------------
namespace d2s {
namespace {
enum { ACT_F32 = 0, ACT_BF16 = 1, ACT_BX3 = 2, ACT_E4M3 = 3 };   // activation formats the engine's producers write
size_t act_bytes(int fmt) { return fmt == ACT_BF16 ? 2 : (fmt == ACT_E4M3 ? 1 : 4); }

// an activation matrix [M, K] (device fp32) as the engine's producers leave it, rows lda elements apart (zero padded): bf16 (RNE), the
// pre-split bf16x3 units, e4m3 of x * qscale (RNE, saturating at +-448: the LayerNorm kernel's / GELU epilogue's conversion) or fp32
int act_operand(ProbeBuf& buf, const float* x, int M, int K, int lda, int fmt, float qscale) {
    std::vector<float> h;
    int rc = fetch_f32(h, x, (size_t)M * K);
    if (rc != D2S_OK) return rc;
    std::vector<uint8_t> o((size_t)M * lda * act_bytes(fmt), 0);
    for (int m = 0; m < M; ++m)
        for (int k = 0; k < K; ++k) {
            const float v = h[(size_t)m * K + k];
            const size_t i = (size_t)m * lda + k;
            if (fmt == ACT_BF16) ((bf16_t*)o.data())[i] = f2bf(v);
            else if (fmt == ACT_E4M3) o[i] = f2e4m3(v * qscale);
            else if (fmt == ACT_BX3) bx3_pack_elem(o.data() + (size_t)m * lda * 4, k, v);
            else ((float*)o.data())[i] = v;
        }
    return upload(buf, o.data(), o.size());
}

}  // namespace
}  // namespace d2s

extern "C" int d2s_linear_probe(d2s_linear_probe_params* p, void* stream) {
    D2S_REQUIRE(p && p->struct_size == sizeof(d2s_linear_probe_params), "d2s_linear_probe_params.struct_size must be sizeof(d2s_linear_probe_params)");
    p->kernel[0] = 0; p->kernel2[0] = 0; p->stats_slots = 0;
    const int prec = p->precision, site = p->site, M = p->M, N = p->N, K = p->K;
    D2S_REQUIRE(prec == D2S_PREC_FP32 || prec == D2S_PREC_BF16 || prec == D2S_PREC_BF16X3 || prec == D2S_PREC_FP8 || prec == D2S_PREC_FP8_MLP, "bad precision");
    D2S_REQUIRE(site >= D2S_LIN_PATCH && site <= D2S_LIN_TM_PROJ_OUT, "bad site");
    D2S_REQUIRE(M > 0 && N > 0 && K > 0 && p->w, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const PrecRules pr = prec_rules(prec);
    const int wprec = pr.w, aprec = pr.act;
    const bool x3 = wprec == D2S_PREC_BF16X3, f8 = pr.e4m3;
    const bool enc = site == D2S_LIN_QKV || site == D2S_LIN_PROJ || site == D2S_LIN_FC1 || site == D2S_LIN_FC2;
    const bool e8 = pr.e4m3_site(site);                                              // this linear runs on e4m3 operands
    const bool fold = p->ln_fold != 0;
    const bool consumer = fold && (site == D2S_LIN_QKV || site == D2S_LIN_FC1 || site == D2S_LIN_NECK_PROJ || site == D2S_LIN_TM_KVQ || site == D2S_LIN_TM_FF1);
    const bool producer = fold && !consumer;
    D2S_REQUIRE(!producer || site == D2S_LIN_PROJ || site == D2S_LIN_FC2 || site == D2S_LIN_TM_PROJ_IN || site == D2S_LIN_TM_TO_OUT || site == D2S_LIN_TM_FF2,
                "ln_fold: not a LayerNorm consumer or producer site");
    // where the engine folds (ln_folds); on the e4m3 precisions the encoder's folds only: an e4m3 engine packs its temporal modules'
    // folded copies but never runs them (d2s_engine_calibrate refuses a temporal engine), and the e4m3 formats below are the encoder's
    D2S_REQUIRE(!fold || (pr.ln_folds(site) && (enc || !f8)), "ln_fold: the engine does not fold LayerNorm there in this precision");
    const bool per_frame = site == D2S_LIN_QKV || site == D2S_LIN_PATCH || site == D2S_LIN_NECK_PROJ;
    const int P = p->ntok - 1;
    D2S_REQUIRE(!per_frame || (p->ntok > 1 && M % (site == D2S_LIN_PATCH ? P : p->ntok) == 0), "M must be a multiple of the rows per frame");
    const int B = per_frame ? M / (site == D2S_LIN_PATCH ? P : p->ntok) : 1;
    D2S_REQUIRE(site != D2S_LIN_QKV || (p->vt && p->heads > 0 && N == 3 * K && K == 64 * p->heads && p->npad >= p->ntok), "QKV: N = 3 K, K = 64 heads, vt, npad >= ntok");
    D2S_REQUIRE(site != D2S_LIN_NECK_RESIZE || (p->ks > 0 && p->gh > 0 && p->gw > 0 && N == p->ks * p->ks * K && M % (p->gh * p->gw) == 0), "NECK_RESIZE: N = ks^2 K, M = B gh gw");
    D2S_REQUIRE(site != D2S_LIN_TM_FF1 || !consumer || N % 8 == 0, "GEGLU: N must be a multiple of 8");
    D2S_REQUIRE(!x3 || (site != D2S_LIN_QKV && site != D2S_LIN_FC1) || (N % 8 == 0 && K % 8 == 0), "bf16x3 unit-format outputs: whole units (N % 8 == 0)");
    D2S_REQUIRE(!consumer || (p->pa && p->pw && p->pK > 0 && p->ln_g && p->ln_b && p->x && p->out2 && p->stats), "ln_fold consumer: pa, pw, ln_g, ln_b, x, out2, stats");
    D2S_REQUIRE(!producer || (p->out2 && (site == D2S_LIN_TM_FF2 || p->stats)), "ln_fold producer: out2, stats");
    const bool x_out = site == D2S_LIN_PATCH || site == D2S_LIN_PROJ || site == D2S_LIN_FC2 || site == D2S_LIN_TM_PROJ_IN || site == D2S_LIN_TM_TO_OUT || site == D2S_LIN_TM_FF2;
    D2S_REQUIRE(x_out ? p->x != nullptr : p->out != nullptr, "x (residual-stream sites) / out needed");
    // the engine's own upload and launch (linear_site.h upload_linear, launch_linear), with e->splitk_ws and device memory of this call:
    // e4m3 forms get deq = s_a * s_w at once, as d2s_engine_calibrate would set it
    ProbeBuf ws;
    if (p->splitk_elems > 0) { int rc = alloc_splitk_ws(ws, (size_t)p->splitk_elems, st); if (rc != D2S_OK) return rc; }
    std::deque<ProbeBuf> mem;
    auto put = [&](LinearImage im, DevLinear& L, float s_a) {
        auto alloc = [&](void** d, const void* h, size_t bytes) { mem.emplace_back(); int rc = upload(mem.back(), h, bytes); *d = mem.back().p; return rc; };
        const bool folded = !im.csum.empty();
        return upload_linear(alloc, std::move(im), L, folded, nullptr, &s_a);
    };
    auto launch = [&](const GemmA& a, const DevLinear& L, int rows, const GemmEpi& ep, char* name) -> int {
        kernel_note() = KernelNote{nullptr, 0, 1, NOTE_TAIL_NONE};
        const int rc = launch_linear(L, a, rows, ep, (float*)ws.p, ws.p ? (size_t)p->splitk_elems : 0, p->tile, st);
        if (rc == D2S_OK) snprintf(name, 128, "%s", noted_kernel().c_str());
        return rc;
    };
    // the raw residual copy: bf16, the unit format (bf16x3), e4m3 of v / s_res where an e4m3 linear consumes it
    const int ofmt = x3 ? ACT_BX3 : ((consumer ? e8 : f8) ? ACT_E4M3 : ACT_BF16);
    const float o2q = ofmt == ACT_E4M3 ? 1.0f / p->s_res : 0.f;
    // ---- the producer of a LayerNorm-folded consumer: the residual update x += pscale * (pa pW^T + pbias) -> out2, stats, slots
    int slots = 0;
    ProbeBuf dPa;
    DevLinear Lp;
    if (consumer) {
        const bool p8 = pr.e4m3_attn;                      // (all-four e4m3: FC2 / proj on e4m3 operands; MLP-only: proj in bf16)
        const int pK = p->pK, D = K;
        std::vector<float> hw, hb;
        int rc = fetch_f32(hw, p->pw, (size_t)D * pK);
        if (rc == D2S_OK && p->pbias) rc = fetch_f32(hb, p->pbias, D);
        if (rc != D2S_OK) return rc;
        rc = put(prepare_linear(p8 ? D2S_PREC_FP8_OPERANDS : wprec, D, pK, [&](int n, int k) { return hw[(size_t)n * pK + k]; }, p->pbias ? hb.data() : nullptr),
                 Lp, p->s_pact);
        if (rc != D2S_OK) return rc;
        const int pfmt = p8 ? ACT_E4M3 : (x3 ? ACT_BX3 : (aprec == D2S_PREC_BF16 ? ACT_BF16 : ACT_F32));
        rc = act_operand(dPa, p->pa, M, pK, pK, pfmt, p8 ? 1.0f / p->s_pact : 0.f);
        if (rc != D2S_OK) return rc;
        GemmA a = {}; a.ptr = dPa.p; a.mode = A_PLAIN; a.lda = pK; a.bx3 = pfmt == ACT_BX3;
        GemmEpi ep = epi_residual(p->x, D, Lp.bias, p->pscale);
        epi_ln_producer(ep, p->out2, p->stats, &slots, x3, o2q);
        rc = launch(a, Lp, M, ep, p->kernel2);
        if (rc != D2S_OK) return rc;
        p->stats_slots = slots;
        if (slots < 1 || slots > 16) { set_error("d2s_linear_probe: the producer leaves no statistics a consumer takes (the engine runs the LayerNorm kernel)"); return D2S_E_UNSUPPORTED; }
    }
    // ---- this linear's weights, in the packed row order: pack_convT's taps, the GEGLU interleave (x | gate in groups of four), else W's own
    DevLinear L;
    {
        std::vector<float> hw, hb, hg, hbt, pb;
        const int Co = site == D2S_LIN_NECK_RESIZE ? K : 0, ks = p->ks;
        int rc = fetch_f32(hw, p->w, (size_t)N * K);
        if (rc == D2S_OK && p->bias) rc = fetch_f32(hb, p->bias, Co ? Co : N);
        if (rc == D2S_OK && consumer) rc = fetch_f32(hg, p->ln_g, K);
        if (rc == D2S_OK && consumer) rc = fetch_f32(hbt, p->ln_b, K);
        if (rc != D2S_OK) return rc;
        const bool geglu = consumer && site == D2S_LIN_TM_FF1;
        auto row = [&](int n) { return geglu ? geglu_row(n, N / 8) : n; };
        auto at = [&](int n, int k) { return Co ? hw[convT_weight_index(n, k, Co, ks)] : hw[(size_t)row(n) * K + k]; };
        if (p->bias) { pb.resize(N); for (int n = 0; n < N; ++n) pb[n] = Co ? hb[n % Co] : hb[row(n)]; }
        rc = put(prepare_linear(e8 ? D2S_PREC_FP8_OPERANDS : wprec, N, K, at, p->bias ? pb.data() : nullptr, consumer ? hg.data() : nullptr,
                                consumer ? hbt.data() : nullptr), L, consumer ? p->s_res : p->s_act);
        if (rc != D2S_OK) return rc;
    }
    // ---- A: the producer's raw residual copy (folded consumers), else the operand as its producer in the engine writes it
    ProbeBuf dA, dR, dR2;
    const int afmt = consumer ? ofmt : (e8 ? ACT_E4M3 : (x3 && enc ? ACT_BX3 : (aprec == D2S_PREC_BF16 ? ACT_BF16 : ACT_F32)));
    int rows = site == D2S_LIN_NECK_PROJ ? B * P : M;
    const int lda = site == D2S_LIN_PATCH ? L.Kpad : K;                                // patchify's rows: Kpad, zero padded
    if (!consumer) {
        D2S_REQUIRE(p->a, "a needed");
        int rc = act_operand(dA, p->a, rows, K, lda, afmt, e8 ? 1.0f / p->s_act : 0.f);
        if (rc != D2S_OK) return rc;
    }
    GemmA a = {}; a.ptr = consumer ? p->out2 : dA.p; a.mode = A_PLAIN; a.lda = lda; a.bx3 = afmt == ACT_BX3;
    // ---- the epilogue, as the engine's launch site builds it
    const float* bias = L.bias;
    GemmEpi ep = {};
    switch (site) {
        case D2S_LIN_PATCH: ep = epi_patch_embed(p->x, N, bias, p->res, P, p->ntok); break;
        case D2S_LIN_QKV: ep = epi_qkv(p->out, qkv_out_type(f8, x3), K, bias, p->vt, p->ntok, p->npad, p->heads); break;
        case D2S_LIN_PROJ: case D2S_LIN_FC2: ep = epi_residual(p->x, N, bias, p->scale); break;
        case D2S_LIN_TM_TO_OUT: case D2S_LIN_TM_FF2: ep = epi_residual(p->x, N, bias, nullptr); break;
        case D2S_LIN_TM_PROJ_IN: ep = rowsE(p->x, OUT_F32, N, bias); break;
        case D2S_LIN_FC1: ep = epi_fc1(p->out, fc1_out_type(x3), N, bias); if (e8) ep.out_qscale = 1.0f / p->s_out; break;
        case D2S_LIN_NECK_RESIZE: ep = epi_convT(p->out, K, bias, p->gh, p->gw, p->ks); break;
        case D2S_LIN_TM_FF1:
            if (consumer) { ep = rowsE(p->out, OUT_T, N / 2, bias); ep.act = ACT_GEGLU; }
            else ep = rowsE(p->out, OUT_T, N, bias);
            break;
        case D2S_LIN_TM_PROJ_OUT: {
            ep = rowsE(p->out, OUT_T, N, bias);
            const int rfmt = aprec == D2S_PREC_BF16 ? ACT_BF16 : ACT_F32;               // residuals: the output's type
            if (p->res) { int rc = act_operand(dR, p->res, M, N, N, rfmt, 0.f); if (rc != D2S_OK) return rc; ep.res1 = dR.p; }
            if (p->res2) { int rc = act_operand(dR2, p->res2, M, N, N, rfmt, 0.f); if (rc != D2S_OK) return rc; ep.res2 = dR2.p; }
            break;
        }
        default: ep = rowsE(p->out, OUT_T, N, bias); break;                             // NECK_PROJ, TM_KVQ
    }
    if (producer) {
        if (site == D2S_LIN_TM_FF2) epi_ln_producer(ep, p->out2, nullptr, nullptr);
        else epi_ln_producer(ep, p->out2, p->stats, &slots, x3, o2q);
    }
    if (consumer) {
        epi_ln_consumer(ep, p->stats, slots, L.csum, p->ln_eps, K);
        rows = M;
        if (site == D2S_LIN_NECK_PROJ) {
            const int skip = epi_tap_fold_rows(ep, B, p->ntok, P);
            a.ptr = (const uint8_t*)p->out2 + (size_t)skip * K * act_bytes(afmt);
            if (skip) rows = P;
        }
    }
    int rc = launch(a, L, rows, ep, p->kernel);
    hipError_t err = hipStreamSynchronize(st);
    if (rc != D2S_OK) return rc;
    D2S_HIP(err);
    if (producer) p->stats_slots = slots;
    return D2S_OK;
}

#ifdef D2S_GLDS_TIMING
extern "C" int d2s_glds_timing(unsigned long long* out, int clear) {      // out != null: read 4096 x 8 stamps
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(d2s::glds_timing), sizeof(unsigned long long) * 4096 * 8) != hipSuccess) return 1;
    if (clear) { static unsigned long long zeros[4096 * 8]; return hipMemcpyToSymbol(HIP_SYMBOL(d2s::glds_timing), zeros, sizeof(zeros)) != hipSuccess; }
    return 0;
}
#endif
