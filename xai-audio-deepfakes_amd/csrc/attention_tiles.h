// The stages of the forward attention kernels (attention.hip), each written once.  A wavefront owns a 16-query tile and computes
// S^T = K Q^T with the KEY on the MFMA row, so a lane ends up with 4 scores per key tile of ONE query: the row max / sum are
// register reductions plus two cross-lane steps, and the P registers are already the B operand of O^T = V^T P^T
// (cdna_hip_programming.md §3 "An accumulator tile as the next MFMA's operand": the k order inside a 32-key step is permuted, and
// V^T is read from LDS in that same order).  Lane coordinates throughout: fr = lane & 15, g = lane >> 4.
//
// What differs between the kernels is a compile-time parameter: NT key tiles, D = head dim rounded up to a multiple of 32 (MFMA k
// step), NTH threads, and NP operand planes -- 1: plain fp16; 2: the split format of device_math.h (hi and lo plane), whose
// products cost three MFMAs per fragment pair.  Arrays of NP fragments are indexed [0] = hi / main, [1] = lo / cross.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "device_math.h"
#include "attention_f32_tiles.h"                 // LOG2E, f32x4

namespace advh {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __fp16 trvec __attribute__((__vector_size__(4 * sizeof(__fp16))));
#define GLOBAL_PTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

// ---------------------------------------------------------------------------------------------------------------- products
// acc += A B.  Two planes: hi*hi into the main accumulator, hi*lo + lo*hi into the cross accumulator (2^-11), issued in the
// order cross(a_hi, b_lo), main(a_hi, b_hi), cross(a_lo, b_hi).
template <int NP>
__device__ __forceinline__ void mma(f32x4 (&acc)[NP], const f16x8 (&a)[NP], const f16x8 (&b)[NP]) {
    if constexpr (NP == 2) {
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0], b[1], acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0], b[0], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[1], b[0], acc[1], 0, 0, 0);
    } else {
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0], b[0], acc[0], 0, 0, 0);
    }
}

template <int NP>
__device__ __forceinline__ float joined(const f32x4 (&acc)[NP], int r) {
    if constexpr (NP == 2) return fmaf(acc[1][r], SPLIT_LO_INV, acc[0][r]);
    else return acc[0][r];
}

// ----------------------------------------------------------------------------------------------------------------- staging
// Eight fp16 zeros in registers of their own.  With a plain constant the compiler shares one zero register among several uses, and
// where a staging register's zero was shared, the word loaded over it had to be copied: a vmcnt wait between the staging loads.
// This steers one compiler's register allocator and can go (a plain f16x8{0, ...} in stage_regs) once that no longer happens.  The
// check: in the device assembly (hipcc --offload-device-only -S) of the register-staged instances, count the s_waitcnt vmcnt that
// stand between two global_load_dwordx4 of one staging pass; with own_zero 7 instances have one, with the plain constant 15.
__device__ __forceinline__ f16x8 own_zero() {
    unsigned w[4];
    asm volatile("v_mov_b32 %0, 0\n\tv_mov_b32 %1, 0\n\tv_mov_b32 %2, 0\n\tv_mov_b32 %3, 0" : "=v"(w[0]), "=v"(w[1]), "=v"(w[2]), "=v"(w[3]));
    f16x8 z;
    __builtin_memcpy(&z, w, 16);
    return z;
}

// Through registers: KEYS keys from key k0 on, K row-major with its 16-byte chunks XOR-swizzled by the row, V transposed (Vd[d][key],
// row pitch VP incl. the per-8-rows skew that spreads the transposing stores over the banks); keys >= T and chunks >= chm are zero.
// NTEN = 2: src is K and V lies vdist elements behind it, both go through registers together; NTEN = 1: src is the one tensor of
// this pass, V if isv.  All global loads of this thread are issued before the first LDS store: one memory latency per workgroup
// instead of one per loop iteration (the transposing stores are scalar and would otherwise serialise behind each load).
template <int KEYS, int D, int NTH, int NTEN>
__device__ __forceinline__ void stage_regs(_Float16* Kd, _Float16* Vd, const _Float16* src, int vdist, bool isv, long ld, int chm, int T,
                                           int k0, int tid) {
    constexpr int CH = D / 8, VP = KEYS + 64, NIT = (KEYS * CH + NTH - 1) / NTH;
    f16x8 reg[NIT][NTEN];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int i = tid + it * NTH, key = i / CH, c = i % CH;
#pragma unroll
        for (int n = 0; n < NTEN; ++n) reg[it][n] = own_zero();
        if (i < KEYS * CH && k0 + key < T && c < chm) {
#pragma unroll
            for (int n = 0; n < NTEN; ++n) reg[it][n] = *(const f16x8*)(src + (long)(k0 + key) * ld + n * vdist + c * 8);
        }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int i = tid + it * NTH, key = i / CH, c = i % CH;
        if (i >= KEYS * CH) break;
        if (NTEN == 2 || !isv) *(f16x8*)(Kd + key * D + ((c ^ (key & (CH - 1))) * 8)) = reg[it][0];
        if (NTEN == 2 || isv) {
#pragma unroll
            for (int j = 0; j < 8; ++j) Vd[(c * 8 + j) * VP + (c & 7) * 8 + key] = reg[it][NTEN - 1][j];
        }
    }
}

// Head dim 64 by the LDS DMA: K and V both ROW-major, plane p at p * NKEY * 128 bytes, chunk c of key r at slot c ^ (r & 7) -- the
// layout stage_regs gives K.  No register round trip, no scalar transposing stores, no V^T buffer (read_v_tr transposes on the
// way out).  Keys >= T re-read key T-1: finite, masked by the softmax / multiplied by P = 0.
template <int NKEY, int NTH, int NP>
__device__ __forceinline__ void stage_dma(char* Ks, char* Vs, const _Float16* base, long lo, long ld, int H, int T, int tid) {
    constexpr int CH = 8, PLB = NKEY * 64 * 2;
    const int lane = tid & 63;
    for (int i = tid; i < NKEY * CH; i += NTH) {
        const int key = i / CH, c = (i % CH) ^ (key & 7);
        const _Float16* src = base + (long)min(key, T - 1) * ld + c * 8;
        const size_t dst = (size_t)(i - lane) * 16;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int p = 0; p < NP; ++p)
                __builtin_amdgcn_global_load_lds(GLOBAL_PTR(src + p * lo + (t + 1) * H), LDS_PTR((t ? Vs : Ks) + p * PLB + dst), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ------------------------------------------------------------------------------------------------------------------ scores
// Q fragments of the query row at row_off: chunks beyond the real head dim (chm chunks of 8) are zero, and so is every chunk of a
// wavefront that is not live.
template <int KK, int NP>
__device__ __forceinline__ void load_q(f16x8 (&q)[KK][NP], const _Float16* base, long lo, long row_off, int g, int chm, bool live) {
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
        const bool in = live && kk * 4 + g < chm;
#pragma unroll
        for (int p = 0; p < NP; ++p) q[kk][p] = in ? *(const f16x8*)(base + p * lo + row_off + kk * 32 + g * 8) : f16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
}

// S^T tiles: rows = keys (4g + r within the tile), column = this lane's query.  Plane p of K lies NT * 16 * D elements behind Ks.
template <int NT, int D, int NP>
__device__ __forceinline__ void score_tiles(f32x4 (&s)[NT], const _Float16* Ks, const f16x8 (&q)[D / 32][NP], int fr, int g) {
    constexpr int CH = D / 8, KK = D / 32, KPL = NT * 16 * D;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
        f32x4 acc[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) acc[p] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const int key = kt * 16 + fr, c = kk * 4 + g;
            const int o = key * D + ((c ^ (key & (CH - 1))) * 8);
            f16x8 k[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) k[p] = *(const f16x8*)(Ks + p * KPL + o);
            mma<NP>(acc, k, q[kk]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kt][r] = joined<NP>(acc, r);
        if ((kt & 1) == 1) __builtin_amdgcn_sched_barrier(0);       // keep the K-fragment reads from being hoisted en bloc (VGPR pressure)
    }
}

// ----------------------------------------------------------------------------------------------------------------- softmax
// Scores of keys k0 .. into the log2 domain (exp(x) = v_exp_f32(x log2 e)), keys >= T to -inf; returns the row maximum.
template <int NT>
__device__ __forceinline__ float mask_scale_max(f32x4 (&s)[NT], float scale, int k0, int T, int g) {
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = (k0 + kt * 16 + g * 4 + r < T) ? s[kt][r] * (scale * LOG2E) : -INFINITY;
            s[kt][r] = v;
            mx = fmaxf(mx, v);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    return fmaxf(mx, __shfl_xor(mx, 32, 64));
}

// s <- 2^(s - sub); returns the row sum.  FAST: the bare v_exp_f32 (fp16 entry); otherwise exp2f (fp32-class entry).
template <int NT, bool FAST>
__device__ __forceinline__ float exp_sum(f32x4 (&s)[NT], float sub) {
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = FAST ? __builtin_amdgcn_exp2f(s[kt][r] - sub) : exp2f(s[kt][r] - sub);
            s[kt][r] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 16, 64);
    return sum + __shfl_xor(sum, 32, 64);
}

// P of the 32-key step ss as the B operand: elements 0-3 from tile 2 ss, 4-7 from tile 2 ss + 1 (zero if NT is odd and this is the
// last step).  NORM: multiplied by inv first.
template <int NT, int NP, bool NORM>
__device__ __forceinline__ void pack_p(f16x8 (&p)[NP], const f32x4 (&s)[NT], int ss, float inv) {
    const bool two = 2 * ss + 1 < NT;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float s0 = s[2 * ss][r], s1 = s[two ? 2 * ss + 1 : 0][r];
        const float e0 = NORM ? s0 * inv : s0, e1 = NORM ? s1 * inv : s1;
        if constexpr (NP == 2) {
            _Float16 h0, l0, h1 = (_Float16)0.f, l1 = (_Float16)0.f;
            split_f32_raw(e0, h0, l0);
            if (two) split_f32_raw(e1, h1, l1);
            p[0][r] = h0; p[1][r] = l0; p[0][4 + r] = h1; p[1][4 + r] = l1;
        } else {
            p[0][r] = (_Float16)e0;
            p[0][4 + r] = two ? (_Float16)e1 : (_Float16)0.f;
        }
    }
}

// --------------------------------------------------------------------------------------------------------------------- P V
// V^T fragment (A operand) of step ss, dims dt * 16 .., plane p, in the key order of pack_p: from the V^T buffer of stage_regs ...
template <int NT, int D>
struct read_v_t {
    const _Float16* Vt;
    int fr, g;
    __device__ __forceinline__ f16x8 operator()(int ss, int dt, int p) const {
        constexpr int VP = NT * 16 + 64;
        const _Float16* vr = Vt + p * D * VP + (dt * 16 + fr) * VP + (((dt * 16 + fr) >> 3) & 7) * 8 + ss * 32 + g * 4;
        const f16x4 lo = *(const f16x4*)vr;
        const f16x4 hi = (2 * ss + 1 < NT) ? *(const f16x4*)(vr + 16) : f16x4{0, 0, 0, 0};
        return f16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
};

// ... or from the row-major V of stage_dma with the transposing LDS load ds_read_b64_tr_b16: lane i of a 16-lane group receives dim
// d0 + i of four consecutive keys, and the key order (4g + q | 16 + 4g + q) of the two reads is exactly the order the P registers
// already have.  A missing odd tile re-reads the even one (P = 0).
template <int NT>
struct read_v_tr {
    const __attribute__((address_space(3))) char* Vs;
    int lane;
    __device__ __forceinline__ f16x8 operator()(int ss, int dt, int p) const {
        constexpr int CH = 8, PLB = NT * 16 * 64 * 2;
        const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
        const int ra = 32 * ss + 4 * g + q, rb = (2 * ss + 1 < NT) ? ra + 16 : ra;
        const int chn = dt * 2 + (pp >> 1), sub = (pp & 1) * 8;
        trvec half[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = h ? rb : ra;
            half[h] = __builtin_amdgcn_ds_read_tr16_b64_v4f16(
                (__attribute__((address_space(3))) trvec*)(Vs + p * PLB + ((size_t)row * CH + (chn ^ (row & 7))) * 16 + sub));
        }
        f16x8 v;
        __builtin_memcpy(&v, half, 16);
        return v;
    }
};

// O^T += V^T P^T for one 32-key step: key steps outermost in the caller, so only one step's V^T fragments are live at a time.
template <int DT, int NP, class VRead>
__device__ __forceinline__ void pv_step(f32x4 (&o)[DT][NP], const f16x8 (&p)[NP], int ss, const VRead& read_v) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        f16x8 v[NP];
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) v[pl] = read_v(ss, dt, pl);
        mma<NP>(o[dt], v, p);
    }
    __builtin_amdgcn_sched_barrier(0);
}

// This lane's four dims of every 16-dim tile to row (element offset) of ctx; dims >= dm are skipped.  NORM: multiplied by inv first.
template <int DT, int NP, bool NORM>
__device__ __forceinline__ void store_ctx(_Float16* ctx, long ctx_lo, long row, const f32x4 (&o)[DT][NP], int g, int dm, float inv) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        if (dt * 16 + g * 4 >= dm) continue;
        if constexpr (NP == 2) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = NORM ? joined<NP>(o[dt], r) * inv : joined<NP>(o[dt], r);
            store_h_rt<4>(ctx, row + dt * 16 + g * 4, ctx_lo, v);
        } else {
            const f16x4 hv = {(_Float16)o[dt][0][0], (_Float16)o[dt][0][1], (_Float16)o[dt][0][2], (_Float16)o[dt][0][3]};
            *(f16x4*)(ctx + row + dt * 16 + g * 4) = hv;
        }
    }
}

// ------------------------------------------------------------------------------------------------- one query tile, single pass
// All keys of the (clip, head) are in LDS, so the softmax needs no online rescaling: scores, softmax, P normalised by 1 / sum, P V,
// store.  base / ctx point at the (clip, head)'s first row; H is ctx's row stride.
template <int NT, int D, int NP, class VRead>
__device__ __forceinline__ void attend_tile(const _Float16* base, long qkv_lo, long ld, const _Float16* Ks, const VRead& read_v, _Float16* ctx,
                                            long ctx_lo, int H, int T, int dm, float scale, int qt, int fr, int g) {
    constexpr int NS = (NT + 1) / 2, KK = D / 32, DT = D / 16;
    const int qrow = qt * 16 + fr;
    const int qr = qrow < T ? qrow : T - 1;
    f16x8 q[KK][NP];
    load_q<KK, NP>(q, base, qkv_lo, (long)qr * ld, g, dm / 8, true);
    f32x4 s[NT];
    score_tiles<NT, D, NP>(s, Ks, q, fr, g);
    const float mx = mask_scale_max<NT>(s, scale, 0, T, g);
    const float inv = 1.f / exp_sum<NT, NP == 1>(s, mx);
    f16x8 p[NS][NP];
#pragma unroll
    for (int ss = 0; ss < NS; ++ss) pack_p<NT, NP, true>(p[ss], s, ss, inv);
    f32x4 o[DT][NP];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) o[dt][pl] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ss = 0; ss < NS; ++ss) pv_step<DT, NP>(o, p[ss], ss, read_v);
    if (qrow < T) store_ctx<DT, NP, false>(ctx, ctx_lo, (long)qrow * H, o, g, dm, 1.f);
}

}  // namespace advh
