// Attention backward of a ragged batch: the ragged siblings of attention_bwd_kernel (backward.hip), attention_bwd_x3_kernel
// (attention_bwd_x3.hip) and attention_bwd_f32_kernel (attention_bwd_f32.hip), one per compiled instance of each.
//
// frames: int32 [B] on the device, clip b has frames[b] valid rows of its Ts.  In the siblings T is both the clip stride
// (b * T * ld) and the bound of every staging loop, tile loop, key mask, row clamp and store.  Here Ts stays the stride (and picks
// the instance class), and T = Tv = clamp(frames[b], 1, Ts) is the bound: rows >= Tv of qkv / dctx are never read for their value,
// rows Tv <= t < Ts of this head's columns of dq | dk | dv are written as zeros (every plane) as the FIRST thing the workgroup does
// (the stores retire behind the staging loads; no register outlives them), and everything between is the sibling's text, reduction
// for reduction: padded keys and queries contribute exact zeros, so frames[b] = Ts reproduces the sibling bit for bit and a clip's
// rows do not depend on the batch around it.
//
// The kernels are copies: the bodies of the three siblings live in their .hip files, and moving them into a shared header would
// have touched those files; their device code is required to stay the same instruction for instruction.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "addvisor_hip.h"
#include "common.h"
#include "device_math.h"
#include "attention_f32_tiles.h"

namespace advh {
namespace ragged_bwd {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __fp16 trvec __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef const __attribute__((address_space(3))) char* lds_cptr;
#define ADVH_GLOBAL_PTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define ADVH_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

// frames[b] clamped to [1, Ts]: no content of `frames` moves an access out of clip b's Ts rows
__device__ __forceinline__ int clip_frames(const int* __restrict__ frames, int b, int Ts) {
    const int f = frames[b];
    return f < 1 ? 1 : (f > Ts ? Ts : f);
}

// rows [Tv, Ts) x this head's dm columns of dq | dk | dv (and of the lo plane when lo != 0) = 0
template <int NTH>
__device__ __forceinline__ void zero_tail(_Float16* dbase, long lo, long ld, int H, int Tv, int Ts, int dm, int tid) {
    const int ch = dm / 8, per = 3 * ch;
    const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < (Ts - Tv) * per; i += NTH) {
        const int row = Tv + i / per, j = i % per;
        _Float16* p = dbase + (long)row * ld + (long)(j / ch) * H + (j % ch) * 8;
        *(f16x8*)p = z;
        if (lo) *(f16x8*)(p + lo) = z;
    }
}

// ---------------------------------------------------------------------------------------------- fp16 (backward.hip)
__device__ __forceinline__ f16x8 tr_frag64(const __attribute__((address_space(3))) char* base, int ra, int rb, int c0, int p) {
    const int ch = (c0 >> 3) + (p >> 1), sub = (p & 1) * 8;
    trvec lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) trvec*)(base + ((size_t)ra * 8 + (ch ^ (ra & 7))) * 16 + sub));
    trvec hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) trvec*)(base + ((size_t)rb * 8 + (ch ^ (rb & 7))) * 16 + sub));
    f16x8 r;
    __builtin_memcpy(&r, &lo, 8);
    __builtin_memcpy((char*)&r + 8, &hi, 8);
    return r;
}

template <int NT, int D, bool TR>
__global__ __launch_bounds__(256) void attention_bwd_ragged_kernel(const _Float16* __restrict__ qkv, const _Float16* __restrict__ dctx,
                                                                   _Float16* __restrict__ dqkv, const int* __restrict__ frames, int Ts,
                                                                   int H, int dm, float scale) {
    constexpr int NKEY = NT * 16, CH = D / 8, VP = NKEY + 64, NS = (NT + 1) / 2, KK = D / 32, DT = D / 16;
    constexpr int ROWB = NKEY * D, TRB = TR ? 0 : D * VP;
    static_assert(!TR || D == 64, "the transposing-read path is for head dim 64");
    constexpr bool STAGE_V = D <= 64;
    constexpr int LDSH = TR ? 2 * ROWB
                            : ((STAGE_V ? 2 * ROWB + TRB : ROWB + TRB) > 2 * TRB ? (STAGE_V ? 2 * ROWB + TRB : ROWB + TRB) : 2 * TRB);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    _Float16* Ks = (_Float16*)smem_raw;
    _Float16* Vs = Ks + ROWB;
    _Float16* Kt = STAGE_V ? Vs + ROWB : Vs;
    _Float16* Qt = (_Float16*)smem_raw;
    _Float16* dOt = Qt + TRB;
    float* rmax = (float*)(smem_raw + LDSH * 2);
    float* rinv = rmax + NKEY;
    float* rdel = rinv + NKEY;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int head = blockIdx.x, b = blockIdx.y;
    const int T = clip_frames(frames, b, Ts);                      // the bound; Ts is the clip stride
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * Ts * ld + head * dm;    // q at +0, k at +H, v at +2H
    const _Float16* dob = dctx + (long)b * Ts * H + head * dm;
    _Float16* dbase = dqkv + (long)b * Ts * ld + head * dm;
    zero_tail<256>(dbase, 0, ld, H, T, Ts, dm, tid);
    const int chm = dm / 8;
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const int fr = lane & 15, g = lane >> 4;
    const int tq = (lane >> 2) & 3, tp = lane & 3;
    const auto* smem3 = (const __attribute__((address_space(3))) char*)ADVH_LDS_PTR(smem_raw);

    if (TR) {
        for (int i = tid; i < NKEY * CH; i += 256) {               // rows >= T re-read row T-1: finite, and masked (p = 0) downstream
            const int key = i / CH, c = (i % CH) ^ (key & 7);
            const _Float16* src = base + (long)min(key, T - 1) * ld + c * 8;
            __builtin_amdgcn_global_load_lds(ADVH_GLOBAL_PTR(src + H), ADVH_LDS_PTR((char*)Ks + (size_t)(i - lane) * 16), 16, 0, 0);
            __builtin_amdgcn_global_load_lds(ADVH_GLOBAL_PTR(src + 2 * H), ADVH_LDS_PTR((char*)Vs + (size_t)(i - lane) * 16), 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else
    for (int i = tid; i < NKEY * CH; i += 256) {
        int key = i / CH, c = i % CH;
        f16x8 kv = {0, 0, 0, 0, 0, 0, 0, 0}, vv = kv;
        if (key < T && c < chm) {
            kv = *(const f16x8*)(base + (long)key * ld + H + c * 8);
            vv = *(const f16x8*)(base + (long)key * ld + 2 * H + c * 8);
        }
        int sw = ((c ^ (key & (CH - 1))) * 8);
        *(f16x8*)(Ks + key * D + sw) = kv;
        if (STAGE_V) *(f16x8*)(Vs + key * D + sw) = vv;
#pragma unroll
        for (int j = 0; j < 8; ++j) Kt[(c * 8 + j) * VP + (c & 7) * 8 + key] = kv[j];
    }
    __syncthreads();

    // ------------------------------------------------------------------ pass A: query tiles
    for (int qt = wv; qt * 16 < T; qt += 4) {
        int qrow = qt * 16 + fr;
        int qr = qrow < T ? qrow : T - 1;
        f16x8 qf[KK], of[KK];
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            qf[kk] = (kk * 4 + g < chm) ? *(const f16x8*)(base + (long)qr * ld + kk * 32 + g * 8) : zero8;
            of[kk] = (kk * 4 + g < chm) ? *(const f16x8*)(dob + (long)qr * H + kk * 32 + g * 8) : zero8;
        }
        f32x4 s[NT], dp[NT];
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
            dp[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                int key = kt * 16 + fr, c = kk * 4 + g;
                int sw = ((c ^ (key & (CH - 1))) * 8);
                f16x8 kf = *(const f16x8*)(Ks + key * D + sw);
                f16x8 vf;
                if (STAGE_V) vf = *(const f16x8*)(Vs + key * D + sw);
                else vf = (key < T && c < chm) ? *(const f16x8*)(base + (long)key * ld + 2 * H + c * 8) : zero8;
                s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[kk], s[kt], 0, 0, 0);      // S^T  [key][q]
                dp[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, of[kk], dp[kt], 0, 0, 0);    // dP^T [key][q]
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = (kt * 16 + g * 4 + r < T) ? s[kt][r] * (scale * LOG2E) : -INFINITY;
                s[kt][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) { float e = __builtin_amdgcn_exp2f(s[kt][r] - mx); s[kt][r] = e; sum += e; }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.f / sum;
        float del = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) { s[kt][r] *= inv; del += s[kt][r] * dp[kt][r]; }
        del += __shfl_xor(del, 16, 64);
        del += __shfl_xor(del, 32, 64);
        if (g == 0 && qrow < NKEY) { rmax[qrow] = mx; rinv[qrow] = inv; rdel[qrow] = del; }
        f16x8 dsf[NS];
#pragma unroll
        for (int ss = 0; ss < NS; ++ss)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dsf[ss][r] = (_Float16)(s[2 * ss][r] * (dp[2 * ss][r] - del) * scale);
                dsf[ss][4 + r] = (2 * ss + 1 < NT) ? (_Float16)(s[(2 * ss + 1 < NT) ? 2 * ss + 1 : 0][r] *
                                                                (dp[(2 * ss + 1 < NT) ? 2 * ss + 1 : 0][r] - del) * scale)
                                                   : (_Float16)0.f;
            }
        f32x4 o[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ss = 0; ss < NS; ++ss) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                f16x8 kf;
                if (TR) {
                    const int ra = 32 * ss + 4 * g + tq;
                    kf = tr_frag64(smem3, ra, (2 * ss + 1 < NT) ? ra + 16 : ra, dt * 16, tp);
                } else {
                    const _Float16* kr = Kt + (dt * 16 + fr) * VP + (((dt * 16 + fr) >> 3) & 7) * 8 + ss * 32 + g * 4;
                    f16x4 lo = *(const f16x4*)kr;
                    f16x4 hi = (2 * ss + 1 < NT) ? *(const f16x4*)(kr + 16) : f16x4{0, 0, 0, 0};
                    kf = f16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, dsf[ss], o[dt], 0, 0, 0);     // dQ^T [d][q]
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (qrow < T) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                if (dt * 16 + g * 4 >= dm) continue;
                f16x4 hv = {(_Float16)o[dt][0], (_Float16)o[dt][1], (_Float16)o[dt][2], (_Float16)o[dt][3]};
                *(f16x4*)(dbase + (long)qrow * ld + dt * 16 + g * 4) = hv;
            }
        }
    }
    __syncthreads();

    // ------------------------------------------------------------------ pass B: key tiles
    if (TR) {
        for (int i = tid; i < NKEY * CH; i += 256) {
            const int row = i / CH, c = (i % CH) ^ (row & 7), rr = min(row, T - 1);
            __builtin_amdgcn_global_load_lds(ADVH_GLOBAL_PTR(base + (long)rr * ld + c * 8), ADVH_LDS_PTR((char*)Ks + (size_t)(i - lane) * 16), 16, 0, 0);
            __builtin_amdgcn_global_load_lds(ADVH_GLOBAL_PTR(dob + (long)rr * H + c * 8), ADVH_LDS_PTR((char*)Vs + (size_t)(i - lane) * 16), 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else
    for (int i = tid; i < NKEY * CH; i += 256) {
        int row = i / CH, c = i % CH;
        f16x8 qv = {0, 0, 0, 0, 0, 0, 0, 0}, ov = qv;
        if (row < T && c < chm) {
            qv = *(const f16x8*)(base + (long)row * ld + c * 8);
            ov = *(const f16x8*)(dob + (long)row * H + c * 8);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { Qt[(c * 8 + j) * VP + (c & 7) * 8 + row] = qv[j]; dOt[(c * 8 + j) * VP + (c & 7) * 8 + row] = ov[j]; }
    }
    __syncthreads();
    for (int kt = wv; kt * 16 < T; kt += 4) {
        int krow = kt * 16 + fr;
        int kr = krow < T ? krow : T - 1;
        f16x8 kf[KK], vf[KK];
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            kf[kk] = (kk * 4 + g < chm) ? *(const f16x8*)(base + (long)kr * ld + H + kk * 32 + g * 8) : zero8;
            vf[kk] = (kk * 4 + g < chm) ? *(const f16x8*)(base + (long)kr * ld + 2 * H + kk * 32 + g * 8) : zero8;
        }
        f32x4 dvt[DT], dkt[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) { dvt[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dkt[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        for (int ss = 0; ss < NS; ++ss) {
            f16x8 pf, dsf;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                int qt = 2 * ss + half;
                f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
                int qrow = qt * 16 + fr;
                int qr = qrow < T ? qrow : T - 1;
                if (qt < NT) {
#pragma unroll
                    for (int kk = 0; kk < KK; ++kk) {
                        f16x8 qf = (kk * 4 + g < chm) ? *(const f16x8*)(base + (long)qr * ld + kk * 32 + g * 8) : zero8;
                        f16x8 of = (kk * 4 + g < chm) ? *(const f16x8*)(dob + (long)qr * H + kk * 32 + g * 8) : zero8;
                        s = __builtin_amdgcn_mfma_f32_16x16x32_f16(qf, kf[kk], s, 0, 0, 0);      // S  [q][key]
                        dp = __builtin_amdgcn_mfma_f32_16x16x32_f16(of, vf[kk], dp, 0, 0, 0);    // dP [q][key]
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    int q = qt * 16 + g * 4 + r;
                    float p = 0.f, ds = 0.f;
                    if (qt < NT && q < T && krow < T) {
                        p = __builtin_amdgcn_exp2f(s[r] * (scale * LOG2E) - rmax[q]) * rinv[q];
                        ds = p * (dp[r] - rdel[q]) * scale;
                    }
                    pf[half * 4 + r] = (_Float16)p;
                    dsf[half * 4 + r] = (_Float16)ds;
                }
            }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                f16x8 oa, qa;
                if (TR) {
                    const int ra = 32 * ss + 4 * g + tq, rb = (2 * ss + 1 < NT) ? ra + 16 : ra;
                    qa = tr_frag64(smem3, ra, rb, dt * 16, tp);
                    oa = tr_frag64(smem3 + (size_t)ROWB * 2, ra, rb, dt * 16, tp);
                } else {
                    const _Float16* orow = dOt + (dt * 16 + fr) * VP + (((dt * 16 + fr) >> 3) & 7) * 8 + ss * 32 + g * 4;
                    const _Float16* qrow_ = Qt + (dt * 16 + fr) * VP + (((dt * 16 + fr) >> 3) & 7) * 8 + ss * 32 + g * 4;
                    f16x4 olo = *(const f16x4*)orow, qlo = *(const f16x4*)qrow_;
                    f16x4 ohi = (2 * ss + 1 < NT) ? *(const f16x4*)(orow + 16) : f16x4{0, 0, 0, 0};
                    f16x4 qhi = (2 * ss + 1 < NT) ? *(const f16x4*)(qrow_ + 16) : f16x4{0, 0, 0, 0};
                    oa = f16x8{olo[0], olo[1], olo[2], olo[3], ohi[0], ohi[1], ohi[2], ohi[3]};
                    qa = f16x8{qlo[0], qlo[1], qlo[2], qlo[3], qhi[0], qhi[1], qhi[2], qhi[3]};
                }
                dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(oa, pf, dvt[dt], 0, 0, 0);      // dV^T [d][key]
                dkt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qa, dsf, dkt[dt], 0, 0, 0);     // dK^T [d][key]
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (krow < T) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                if (dt * 16 + g * 4 >= dm) continue;
                f16x4 kv = {(_Float16)dkt[dt][0], (_Float16)dkt[dt][1], (_Float16)dkt[dt][2], (_Float16)dkt[dt][3]};
                f16x4 vv = {(_Float16)dvt[dt][0], (_Float16)dvt[dt][1], (_Float16)dvt[dt][2], (_Float16)dvt[dt][3]};
                *(f16x4*)(dbase + (long)krow * ld + H + dt * 16 + g * 4) = kv;
                *(f16x4*)(dbase + (long)krow * ld + 2 * H + dt * 16 + g * 4) = vv;
            }
        }
    }
}

template <int NT, int D, bool TR>
static int launch_att_bwd(const void* qkv, const void* dctx, void* dqkv, const int* frames, int B, int T, int H, int heads, int dm,
                          float scale, hipStream_t s) {
    constexpr int NKEY = NT * 16, VP = NKEY + 64, ROWB = NKEY * D, TRB = TR ? 0 : D * VP;
    constexpr int PA = TR ? 2 * ROWB : (D <= 64 ? 2 * ROWB + TRB : ROWB + TRB);
    const size_t lds = (size_t)(PA > 2 * TRB ? PA : 2 * TRB) * 2 + 3 * NKEY * 4;
    if (lds > 160 * 1024) return ADVH_EUNSUPPORTED;
    if (advh_ensure_lds((const void*)attention_bwd_ragged_kernel<NT, D, TR>) != ADVH_OK) return ADVH_ELAUNCH;
    hipLaunchKernelGGL((attention_bwd_ragged_kernel<NT, D, TR>), dim3(heads, B), dim3(256), lds, s, (const _Float16*)qkv,
                       (const _Float16*)dctx, (_Float16*)dqkv, frames, T, H, dm, scale);
    return ADVH_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------- split arithmetic (attention_bwd_x3.hip)
template <int NT, int D>
struct AttBwdX3 {
    static constexpr int NS = (NT + 1) / 2, ROWS = NS * 32;
    static constexpr int PLANE = ROWS * D;
    static constexpr int LDS_BYTES = 4 * PLANE * 2 + 3 * ROWS * 4;
};

template <int D> __device__ __forceinline__ int swz(int r, int c) { return r * D + ((c ^ (r & (D / 8 - 1))) << 3); }

template <int ROWS, int D, int NTH>
__device__ __forceinline__ void stage_planes(_Float16* ph, _Float16* pl, const _Float16* src, long lo, long ld, int T, int dm, int tid) {
    constexpr int CH = D / 8;
    for (int i = tid; i < ROWS * CH; i += NTH) {
        const int row = i / CH, c = i % CH;
        f16x8 h = {0, 0, 0, 0, 0, 0, 0, 0}, l = {0, 0, 0, 0, 0, 0, 0, 0};
        if (row < T && c * 8 < dm) {
            h = *(const f16x8*)(src + (long)row * ld + c * 8);
            l = *(const f16x8*)(src + lo + (long)row * ld + c * 8);
        }
        *(f16x8*)(ph + swz<D>(row, c)) = h;
        *(f16x8*)(pl + swz<D>(row, c)) = l;
    }
}

template <int D> __device__ __forceinline__ int tr_off(int g, int fr, int c0) {
    const int q = fr >> 2, p = fr & 3;
    return 2 * swz<D>(4 * g + q, (c0 >> 3) + (p >> 1)) + (p & 1) * 8;
}
template <int D>
__device__ __forceinline__ f16x8 tr8(lds_cptr plane, int off) {
    const auto* pa = (const __attribute__((address_space(3))) trvec*)(plane + off);
    const auto* pb = (const __attribute__((address_space(3))) trvec*)(plane + off + 16 * (2 * D));
    trvec lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) trvec*)pa);
    trvec hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) trvec*)pb);
    f16x8 r;
    __builtin_memcpy(&r, &lo, 8);
    __builtin_memcpy((char*)&r + 8, &hi, 8);
    return r;
}

__device__ __forceinline__ f16x8 gfrag(const _Float16* p, bool in) {
    return in ? *(const f16x8*)p : f16x8{0, 0, 0, 0, 0, 0, 0, 0};
}

#define MFMA_X3(accm, accx, ah, al, bh, bl)                                          \
    do {                                                                             \
        accx = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, accx, 0, 0, 0);        \
        accm = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, accm, 0, 0, 0);        \
        accx = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, accx, 0, 0, 0);        \
    } while (0)
// operand roles exchanged, cross terms in pass A's order (attention_bwd_x3.hip explains why the order matters)
#define MFMA_X3_SWAPPED(accm, accx, ah, al, bh, bl)                                  \
    do {                                                                             \
        accx = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, accx, 0, 0, 0);        \
        accm = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, accm, 0, 0, 0);        \
        accx = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, accx, 0, 0, 0);        \
    } while (0)

template <int NT, int D, int NW>
__global__ __launch_bounds__(64 * NW) void attention_bwd_x3_ragged_kernel(const _Float16* __restrict__ qkv, long qkv_lo,
                                                                          const _Float16* __restrict__ dctx, long dctx_lo,
                                                                          _Float16* __restrict__ dqkv, long dqkv_lo,
                                                                          const int* __restrict__ frames, int Ts, int H, int dm, float scale) {
    typedef AttBwdX3<NT, D> G;
    constexpr int ROWS = G::ROWS, PLANE = G::PLANE, KK = D / 32, DG = D / 16, NS = G::NS;
    extern __shared__ __attribute__((aligned(16))) _Float16 smx[];
    _Float16* P0h = smx;                                  // K (pass A), Q (pass B)
    _Float16* P0l = smx + PLANE;
    _Float16* P1h = smx + 2 * PLANE;                      // V (pass A), dO (pass B)
    _Float16* P1l = smx + 3 * PLANE;
    float* rmax = (float*)(smx + 4 * PLANE);
    float* rinv = rmax + ROWS;
    float* rdel = rinv + ROWS;
    const lds_cptr L0h = (lds_cptr)((__attribute__((address_space(3))) void*)P0h);
    const lds_cptr L0l = L0h + 2 * PLANE, L1h = L0h + 4 * PLANE, L1l = L0h + 6 * PLANE;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y;
    const int T = clip_frames(frames, b, Ts);                            // the bound; Ts is the clip stride
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * Ts * ld + head * dm;          // q at +0, k at +H, v at +2H
    const _Float16* dob = dctx + (long)b * Ts * H + head * dm;
    _Float16* dbase = dqkv + (long)b * Ts * ld + head * dm;
    zero_tail<64 * NW>(dbase, dqkv_lo, ld, H, T, Ts, dm, tid);
    const float c2 = scale * LOG2E;
    const int nst = (T + 31) / 32;
    int troff[DG], rowoff[KK];
#pragma unroll
    for (int dt = 0; dt < DG; ++dt) troff[dt] = tr_off<D>(g, fr, 16 * dt);
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) rowoff[kk] = swz<D>(fr, kk * 4 + g);

    for (int i = tid; i < 3 * ROWS; i += 64 * NW) rmax[i] = 0.f;
    stage_planes<ROWS, D, 64 * NW>(P0h, P0l, base + H, qkv_lo, ld, T, dm, tid);
    stage_planes<ROWS, D, 64 * NW>(P1h, P1l, base + 2 * H, qkv_lo, ld, T, dm, tid);
    __syncthreads();

    // ------------------------------------------------------------------ pass A: query tiles
    for (int qt = wv; qt * 16 < T; qt += NW) {
        const int qrow = qt * 16 + fr, qr = qrow < T ? qrow : T - 1;
        f32x4 s[NT], dp[NT];
        {
            f16x8 qh[KK], ql[KK];
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const int c = kk * 4 + g;
                qh[kk] = gfrag(base + (long)qr * ld + c * 8, c * 8 < dm);
                ql[kk] = gfrag(base + qkv_lo + (long)qr * ld + c * 8, c * 8 < dm);
            }
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) {
                f32x4 sm_ = {0.f, 0.f, 0.f, 0.f}, sx = sm_;
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    const int o = kt * 16 * D + rowoff[kk];
                    const f16x8 kh = *(const f16x8*)(P0h + o), kl = *(const f16x8*)(P0l + o);
                    MFMA_X3(sm_, sx, kh, kl, qh[kk], ql[kk]);          // S^T  [key][q]
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) s[kt][r] = fmaf(sx[r], SPLIT_LO_INV, sm_[r]);
                if ((kt & 1) == 1) __builtin_amdgcn_sched_barrier(0);
            }
        }
        {
            f16x8 oh[KK], ol[KK];
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const int c = kk * 4 + g;
                oh[kk] = gfrag(dob + (long)qr * H + c * 8, c * 8 < dm);
                ol[kk] = gfrag(dob + dctx_lo + (long)qr * H + c * 8, c * 8 < dm);
            }
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) {
                f32x4 pm = {0.f, 0.f, 0.f, 0.f}, px = pm;
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    const int o = kt * 16 * D + rowoff[kk];
                    const f16x8 vh = *(const f16x8*)(P1h + o), vl = *(const f16x8*)(P1l + o);
                    MFMA_X3(pm, px, vh, vl, oh[kk], ol[kk]);           // dP^T [key][q]
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) dp[kt][r] = fmaf(px[r], SPLIT_LO_INV, pm[r]);
                if ((kt & 1) == 1) __builtin_amdgcn_sched_barrier(0);
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = (kt * 16 + g * 4 + r < T) ? s[kt][r] * c2 : -INFINITY;       // log2 domain
                s[kt][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float e = __builtin_amdgcn_exp2f(s[kt][r] - mx); s[kt][r] = e; sum += e; }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.f / sum;
        float del = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) { s[kt][r] *= inv; del += s[kt][r] * dp[kt][r]; }
        del += __shfl_xor(del, 16, 64);
        del += __shfl_xor(del, 32, 64);
        if (g == 0) { rmax[qrow] = mx; rinv[qrow] = inv; rdel[qrow] = del; }                 // qrow < ROWS always
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[kt][r] = s[kt][r] * (dp[kt][r] - del) * scale;     // dS^T [key][q]; 0 for keys >= T (p = 0)
        f32x4 om[DG], ox[DG];
#pragma unroll
        for (int dt = 0; dt < DG; ++dt) { om[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; ox[dt] = om[dt]; }
#pragma unroll
        for (int ss = 0; ss < NS; ++ss) {
            float v[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) { v[r] = s[2 * ss][r]; v[4 + r] = (2 * ss + 1 < NT) ? s[(2 * ss + 1 < NT) ? 2 * ss + 1 : 0][r] : 0.f; }
            f16x8 bh, bl;
            split_f32_vec<8>(v, bh, bl);
#pragma unroll
            for (int dt = 0; dt < DG; ++dt) {
                const f16x8 ah = tr8<D>(L0h, 32 * ss * (2 * D) + troff[dt]), al = tr8<D>(L0l, 32 * ss * (2 * D) + troff[dt]);
                MFMA_X3(om[dt], ox[dt], ah, al, bh, bl);           // dQ^T [d][q] += K^T dS^T
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (qrow < T) {
#pragma unroll
            for (int dt = 0; dt < DG; ++dt) {
                if (dt * 16 + g * 4 >= dm) continue;
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaf(ox[dt][r], SPLIT_LO_INV, om[dt][r]);
                store_h_rt<4>(dbase, (long)qrow * ld + dt * 16 + g * 4, dqkv_lo, v);
            }
        }
    }
    __syncthreads();

    // ------------------------------------------------------------------ pass B: key tiles
    stage_planes<ROWS, D, 64 * NW>(P0h, P0l, base, qkv_lo, ld, T, dm, tid);              // Q
    stage_planes<ROWS, D, 64 * NW>(P1h, P1l, dob, dctx_lo, (long)H, T, dm, tid);         // dO
    __syncthreads();
    for (int kt = wv; kt * 16 < T; kt += NW) {
        const int krow = kt * 16 + fr, kr_ = krow < T ? krow : T - 1;
        f16x8 kh[KK], kl[KK], vh[KK], vl[KK];
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const int c = kk * 4 + g;
            const bool in = c * 8 < dm;
            kh[kk] = gfrag(base + H + (long)kr_ * ld + c * 8, in);
            kl[kk] = gfrag(base + H + qkv_lo + (long)kr_ * ld + c * 8, in);
            vh[kk] = gfrag(base + 2 * H + (long)kr_ * ld + c * 8, in);
            vl[kk] = gfrag(base + 2 * H + qkv_lo + (long)kr_ * ld + c * 8, in);
        }
        f32x4 dkm[DG], dkx[DG], dvm[DG], dvx[DG];
#pragma unroll
        for (int dt = 0; dt < DG; ++dt) { dkm[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dkx[dt] = dkm[dt]; dvm[dt] = dkm[dt]; dvx[dt] = dkm[dt]; }
        for (int ss = 0; ss < nst; ++ss) {
            float p[8], ds[8];
            const int sb = ss * 32 * D;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x4 sm_ = {0.f, 0.f, 0.f, 0.f}, sx = sm_, pm = sm_, px = sm_;
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    const int o = sb + h * 16 * D + rowoff[kk];             // rows >= T are zero in LDS
                    const f16x8 qah = *(const f16x8*)(P0h + o), qal = *(const f16x8*)(P0l + o);
                    const f16x8 oah = *(const f16x8*)(P1h + o), oal = *(const f16x8*)(P1l + o);
                    MFMA_X3_SWAPPED(sm_, sx, qah, qal, kh[kk], kl[kk]);     // S  [q][key], bit-equal to pass A's S^T
                    MFMA_X3_SWAPPED(pm, px, oah, oal, vh[kk], vl[kk]);      // dP [q][key], bit-equal to pass A's dP^T
                }
                const int q0 = ss * 32 + h * 16 + g * 4;
                const float4 mx4 = *(const float4*)(rmax + q0), iv4 = *(const float4*)(rinv + q0), dl4 = *(const float4*)(rdel + q0);
                const float mxs[4] = {mx4.x, mx4.y, mx4.z, mx4.w}, ivs[4] = {iv4.x, iv4.y, iv4.z, iv4.w}, dls[4] = {dl4.x, dl4.y, dl4.z, dl4.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pv = __builtin_amdgcn_exp2f(fmaf(sx[r], SPLIT_LO_INV, sm_[r]) * c2 - mxs[r]) * ivs[r];
                    const float dv = pv * (fmaf(px[r], SPLIT_LO_INV, pm[r]) - dls[r]) * scale;
                    const bool ok = q0 + r < T && krow < T;
                    p[4 * h + r] = ok ? pv : 0.f;
                    ds[4 * h + r] = ok ? dv : 0.f;
                }
            }
            f16x8 ph, pl, dh, dl;
#pragma unroll
            for (int j = 0; j < 8; ++j) { _Float16 a, c; split_f32_raw(p[j], a, c); ph[j] = a; pl[j] = c; }
            split_f32_vec<8>(ds, dh, dl);
#pragma unroll
            for (int dt = 0; dt < DG; ++dt) {
                const int a = 2 * sb + troff[dt];
                const f16x8 qth = tr8<D>(L0h, a), qtl = tr8<D>(L0l, a);
                const f16x8 oth = tr8<D>(L1h, a), otl = tr8<D>(L1l, a);
                MFMA_X3(dkm[dt], dkx[dt], qth, qtl, dh, dl);        // dK^T [d][key] += Q^T dS
                MFMA_X3(dvm[dt], dvx[dt], oth, otl, ph, pl);        // dV^T [d][key] += dO^T P
            }
        }
        if (krow < T) {
#pragma unroll
            for (int dt = 0; dt < DG; ++dt) {
                if (dt * 16 + g * 4 >= dm) continue;
                float kv[4], vv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { kv[r] = fmaf(dkx[dt][r], SPLIT_LO_INV, dkm[dt][r]); vv[r] = fmaf(dvx[dt][r], SPLIT_LO_INV, dvm[dt][r]); }
                store_h_rt<4>(dbase, (long)krow * ld + H + dt * 16 + g * 4, dqkv_lo, kv);
                store_h_rt<4>(dbase, (long)krow * ld + 2 * H + dt * 16 + g * 4, dqkv_lo, vv);
            }
        }
    }
}

template <int NT, int D, int NW>
static int launch_att_bwd_x3(const void* qkv, long qkv_lo, const void* dctx, long dctx_lo, void* dqkv, long dqkv_lo, const int* frames,
                             int B, int T, int H, int heads, int dm, float scale, hipStream_t s) {
    constexpr int lds = AttBwdX3<NT, D>::LDS_BYTES;
    static_assert(lds <= 160 * 1024, "two matrices in two planes must fit");
    if (advh_ensure_lds((const void*)attention_bwd_x3_ragged_kernel<NT, D, NW>) != ADVH_OK) return ADVH_ELAUNCH;
    hipLaunchKernelGGL((attention_bwd_x3_ragged_kernel<NT, D, NW>), dim3(heads, B), dim3(64 * NW), lds, s, (const _Float16*)qkv, qkv_lo,
                       (const _Float16*)dctx, dctx_lo, (_Float16*)dqkv, dqkv_lo, frames, T, H, dm, scale);
    return ADVH_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------- fp32 matrix instruction (attention_bwd_f32.hip)
template <int NT, int D>
struct AttBwdF32 {
    static constexpr int NKEY = NT * 16, PITCH = D + 4, DG = D / 16;
    static constexpr int MAT = NKEY * PITCH;
    static constexpr bool TWO = (2 * MAT + 3 * NKEY) * 4 <= 160 * 1024;
    static constexpr int LDS_BYTES = ((TWO ? 2 : 1) * MAT + 3 * NKEY) * 4;
};

template <int NT, int D, int NW>
__global__ __launch_bounds__(64 * NW) void attention_bwd_f32_ragged_kernel(const _Float16* __restrict__ qkv, long qkv_lo,
                                                                           const _Float16* __restrict__ dctx, long dctx_lo,
                                                                           _Float16* __restrict__ dqkv, long dqkv_lo,
                                                                           const int* __restrict__ frames, int Ts, int H, int dm, float scale) {
    typedef AttBwdF32<NT, D> G;
    constexpr int NKEY = G::NKEY, PITCH = G::PITCH, DG = G::DG;
    constexpr bool TWO = G::TWO;
    extern __shared__ __attribute__((aligned(16))) float smf[];
    float* M0 = smf;                                      // K (pass A), Q (pass B1), dO (pass B2)
    float* M1 = smf + G::MAT;                             // TWO: V (pass A), dO (pass B)
    float* rmax = smf + (TWO ? 2 : 1) * G::MAT;
    float* rinv = rmax + NKEY;
    float* rdel = rinv + NKEY;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int fr = lane & 15, g = lane >> 4;
    const int head = blockIdx.x, b = blockIdx.y;
    const int T = clip_frames(frames, b, Ts);                            // the bound; Ts is the clip stride
    const long ld = 3L * H;
    const _Float16* base = qkv + (long)b * Ts * ld + head * dm;          // q at +0, k at +H, v at +2H
    const _Float16* dob = dctx + (long)b * Ts * H + head * dm;
    _Float16* dbase = dqkv + (long)b * Ts * ld + head * dm;
    zero_tail<64 * NW>(dbase, dqkv_lo, ld, H, T, Ts, dm, tid);
    const float c2 = scale * LOG2E;

    stage_f32<NKEY, D, 64 * NW>(M0, base + H, qkv_lo, ld, T, dm, tid);
    if (TWO) stage_f32<NKEY, D, 64 * NW>(M1, base + 2 * H, qkv_lo, ld, T, dm, tid);
    __syncthreads();

    // ------------------------------------------------------------------ pass A: query tiles
    for (int qt = wv; qt * 16 < T; qt += NW) {
        const int qrow = qt * 16 + fr, qr = qrow < T ? qrow : T - 1;
        float4 qf[DG], of[DG];
#pragma unroll
        for (int G_ = 0; G_ < DG; ++G_) {
            qf[G_] = grow4(base, qkv_lo, (long)qr * ld, 16 * G_ + 4 * g, dm);
            of[G_] = grow4(dob, dctx_lo, (long)qr * H, 16 * G_ + 4 * g, dm);
        }
        f32x4 s[NT], dp[NT];
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
            dp[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int key = kt * 16 + fr, keyc = key < T ? key : T - 1;
#pragma unroll
            for (int G_ = 0; G_ < DG; ++G_) {
                const float4 kf = *(const float4*)(M0 + key * PITCH + 16 * G_ + 4 * g);
                float4 vf;
                if (TWO) vf = *(const float4*)(M1 + key * PITCH + 16 * G_ + 4 * g);
                else vf = grow4(base + 2 * H, qkv_lo, (long)keyc * ld, 16 * G_ + 4 * g, dm);
                MFMA4(s[kt], kf, qf[G_]);                 // S^T  [key][q]
                MFMA4(dp[kt], vf, of[G_]);                // dP^T [key][q]
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = (kt * 16 + g * 4 + r < T) ? s[kt][r] * c2 : -INFINITY;       // log2 domain
                s[kt][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float e = exp2f(s[kt][r] - mx); s[kt][r] = e; sum += e; }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.f / sum;
        float del = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) { s[kt][r] *= inv; del += s[kt][r] * dp[kt][r]; }
        del += __shfl_xor(del, 16, 64);
        del += __shfl_xor(del, 32, 64);
        if (g == 0 && qrow < NKEY) { rmax[qrow] = mx; rinv[qrow] = inv; rdel[qrow] = del; }
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[kt][r] = s[kt][r] * (dp[kt][r] - del) * scale;     // dS^T [key][q]; 0 for keys >= T (p = 0)
        f32x4 o[DG];
#pragma unroll
        for (int dt = 0; dt < DG; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* kr = M0 + (kt * 16 + 4 * g + r) * PITCH + fr;
#pragma unroll
                for (int dt = 0; dt < DG; ++dt)
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[16 * dt], s[kt][r], o[dt], 0, 0, 0);   // dQ^T [d][q]
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (qrow < T) {
#pragma unroll
            for (int dt = 0; dt < DG; ++dt) {
                if (dt * 16 + g * 4 >= dm) continue;
                const float v[4] = {o[dt][0], o[dt][1], o[dt][2], o[dt][3]};
                store_h_rt<4>(dbase, (long)qrow * ld + dt * 16 + g * 4, dqkv_lo, v);
            }
        }
    }
    __syncthreads();

    // ------------------------------------------------------------------ pass B: key tiles
    stage_f32<NKEY, D, 64 * NW>(M0, base, qkv_lo, ld, T, dm, tid);                 // Q
    if (TWO) stage_f32<NKEY, D, 64 * NW>(M1, dob, dctx_lo, (long)H, T, dm, tid);   // dO
    __syncthreads();
    for (int kt = wv; kt * 16 < T; kt += NW) {
        const int krow = kt * 16 + fr, kr_ = krow < T ? krow : T - 1;
        float4 kf[DG], vf[DG];
#pragma unroll
        for (int G_ = 0; G_ < DG; ++G_) {
            kf[G_] = grow4(base + H, qkv_lo, (long)kr_ * ld, 16 * G_ + 4 * g, dm);
            vf[G_] = grow4(base + 2 * H, qkv_lo, (long)kr_ * ld, 16 * G_ + 4 * g, dm);
        }
        f32x4 dkt[DG], dvt[DG];
#pragma unroll
        for (int dt = 0; dt < DG; ++dt) { dkt[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dvt[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        for (int qt = 0; qt * 16 < T; ++qt) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
            const int qrow = qt * 16 + fr, qr = qrow < T ? qrow : T - 1;
#pragma unroll
            for (int G_ = 0; G_ < DG; ++G_) {
                const float4 qa = *(const float4*)(M0 + qrow * PITCH + 16 * G_ + 4 * g);
                float4 oa;
                if (TWO) oa = *(const float4*)(M1 + qrow * PITCH + 16 * G_ + 4 * g);
                else oa = grow4(dob, dctx_lo, (long)qr * H, 16 * G_ + 4 * g, dm);
                MFMA4(s, qa, kf[G_]);                     // S  [q][key]
                MFMA4(dp, oa, vf[G_]);                    // dP [q][key]
            }
            float p[4], ds[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = qt * 16 + g * 4 + r;
                p[r] = 0.f;
                ds[r] = 0.f;
                if (q < T && krow < T) {
                    p[r] = exp2f(s[r] * c2 - rmax[q]) * rinv[q];
                    ds[r] = p[r] * (dp[r] - rdel[q]) * scale;
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* qrw = M0 + (qt * 16 + 4 * g + r) * PITCH + fr;
                const float* orw = M1 + (qt * 16 + 4 * g + r) * PITCH + fr;
#pragma unroll
                for (int dt = 0; dt < DG; ++dt) {
                    dkt[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(qrw[16 * dt], ds[r], dkt[dt], 0, 0, 0);              // dK^T [d][key]
                    if (TWO) dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(orw[16 * dt], p[r], dvt[dt], 0, 0, 0);     // dV^T [d][key]
                }
            }
        }
        if (krow < T) {
#pragma unroll
            for (int dt = 0; dt < DG; ++dt) {
                if (dt * 16 + g * 4 >= dm) continue;
                const float kv[4] = {dkt[dt][0], dkt[dt][1], dkt[dt][2], dkt[dt][3]};
                store_h_rt<4>(dbase, (long)krow * ld + H + dt * 16 + g * 4, dqkv_lo, kv);
                if (TWO) {
                    const float vv[4] = {dvt[dt][0], dvt[dt][1], dvt[dt][2], dvt[dt][3]};
                    store_h_rt<4>(dbase, (long)krow * ld + 2 * H + dt * 16 + g * 4, dqkv_lo, vv);
                }
            }
        }
    }
    if (TWO) return;

    // ------------------------------------------------------------------ pass B2 (one matrix fits): dO staged, dV^T = dO^T P
    __syncthreads();
    stage_f32<NKEY, D, 64 * NW>(M0, dob, dctx_lo, (long)H, T, dm, tid);
    __syncthreads();
    for (int kt = wv; kt * 16 < T; kt += NW) {
        const int krow = kt * 16 + fr, kr_ = krow < T ? krow : T - 1;
        float4 kf[DG];
#pragma unroll
        for (int G_ = 0; G_ < DG; ++G_) kf[G_] = grow4(base + H, qkv_lo, (long)kr_ * ld, 16 * G_ + 4 * g, dm);
        f32x4 dvt[DG];
#pragma unroll
        for (int dt = 0; dt < DG; ++dt) dvt[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int qt = 0; qt * 16 < T; ++qt) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            const int qrow = qt * 16 + fr, qr = qrow < T ? qrow : T - 1;
#pragma unroll
            for (int G_ = 0; G_ < DG; ++G_) {
                const float4 qa = grow4(base, qkv_lo, (long)qr * ld, 16 * G_ + 4 * g, dm);
                MFMA4(s, qa, kf[G_]);
            }
            float p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = qt * 16 + g * 4 + r;
                p[r] = (q < T && krow < T) ? exp2f(s[r] * c2 - rmax[q]) * rinv[q] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* orw = M0 + (qt * 16 + 4 * g + r) * PITCH + fr;
#pragma unroll
                for (int dt = 0; dt < DG; ++dt) dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(orw[16 * dt], p[r], dvt[dt], 0, 0, 0);
            }
        }
        if (krow < T) {
#pragma unroll
            for (int dt = 0; dt < DG; ++dt) {
                if (dt * 16 + g * 4 >= dm) continue;
                const float vv[4] = {dvt[dt][0], dvt[dt][1], dvt[dt][2], dvt[dt][3]};
                store_h_rt<4>(dbase, (long)krow * ld + 2 * H + dt * 16 + g * 4, dqkv_lo, vv);
            }
        }
    }
}

template <int NT, int D>
static int launch_att_bwd_f32(const void* qkv, long qkv_lo, const void* dctx, long dctx_lo, void* dqkv, long dqkv_lo, const int* frames,
                              int B, int T, int H, int heads, int dm, float scale, hipStream_t s) {
    constexpr int lds = AttBwdF32<NT, D>::LDS_BYTES;
    static_assert(lds <= 160 * 1024, "one staged matrix must fit");
    constexpr int NW = D <= 64 ? 8 : 4;
    if (advh_ensure_lds((const void*)attention_bwd_f32_ragged_kernel<NT, D, NW>) != ADVH_OK) return ADVH_ELAUNCH;
    hipLaunchKernelGGL((attention_bwd_f32_ragged_kernel<NT, D, NW>), dim3(heads, B), dim3(64 * NW), lds, s, (const _Float16*)qkv, qkv_lo,
                       (const _Float16*)dctx, dctx_lo, (_Float16*)dqkv, dqkv_lo, frames, T, H, dm, scale);
    return ADVH_LAUNCH_CHECK();
}

}  // namespace ragged_bwd
}  // namespace advh

using namespace advh;
using namespace advh::ragged_bwd;

extern "C" int advh_attention_bwd_f16_ragged(const void* qkv, const void* dctx, void* dqkv, const int32_t* frames, int B, int T, int H,
                                             int heads, advh_stream_t stream) {
    if (!qkv || !dctx || !dqkv || !frames || B <= 0 || T <= 0 || H <= 0 || heads <= 0 || H % heads) return ADVH_EINVAL;
    const int dm = H / heads;
    if (T > 256 || dm % 8 || dm > 128) return ADVH_EUNSUPPORTED;
    const int D = dm <= 32 ? 32 : (dm <= 64 ? 64 : 128);
    const float scale = 1.f / sqrtf((float)dm);
    hipStream_t s = (hipStream_t)stream;
    const int* fv = (const int*)frames;
    const int nt = (T + 15) / 16;                            // the instance class follows the row stride, as in the sibling
#define ATB(NT_, D_) return launch_att_bwd<NT_, D_, false>(qkv, dctx, dqkv, fv, B, T, H, heads, dm, scale, s)
#define ATBT(NT_) return launch_att_bwd<NT_, 64, true>(qkv, dctx, dqkv, fv, B, T, H, heads, dm, scale, s)
    if (dm == 64) { if (nt <= 4) ATBT(4); else if (nt <= 8) ATBT(8); else if (nt <= 13) ATBT(13); else ATBT(16); }
    else if (D == 64) { if (nt <= 4) ATB(4, 64); else if (nt <= 8) ATB(8, 64); else if (nt <= 13) ATB(13, 64); else ATB(16, 64); }
    else if (D == 32) { if (nt <= 4) ATB(4, 32); else if (nt <= 8) ATB(8, 32); else if (nt <= 13) ATB(13, 32); else ATB(16, 32); }
    else { if (nt <= 4) ATB(4, 128); else if (nt <= 13) ATB(13, 128); else ATB(16, 128); }
#undef ATB
#undef ATBT
}

extern "C" int advh_attention_bwd_split_ragged(const void* qkv, int64_t qkv_lo, const void* dctx, int64_t dctx_lo, void* dqkv,
                                               int64_t dqkv_lo, const int32_t* frames, int B, int T, int H, int heads,
                                               advh_stream_t stream) {
    if (!qkv || !dctx || !dqkv || !frames || B <= 0 || T <= 0 || H <= 0 || heads <= 0 || H % heads) return ADVH_EINVAL;
    if (qkv_lo <= 0 || dctx_lo <= 0 || dqkv_lo <= 0 || qkv_lo % 8 || dctx_lo % 8 || dqkv_lo % 8) return ADVH_EINVAL;
    const int dm = H / heads;
    if (T > 256 || dm % 8 || dm > 128) return ADVH_EUNSUPPORTED;
    const int D = dm <= 32 ? 32 : (dm <= 64 ? 64 : 128);
    const float scale = 1.f / sqrtf((float)dm);
    hipStream_t s = (hipStream_t)stream;
    const int* fv = (const int*)frames;
    const int nt = (T + 15) / 16;
    if (dm <= 64 && !g_att_bwd_force_f32) {                  // the split-arithmetic kernel, as advh_attention_bwd_split picks it
#define ATX(NT_, D_, NW_) return launch_att_bwd_x3<NT_, D_, NW_>(qkv, qkv_lo, dctx, dctx_lo, dqkv, dqkv_lo, fv, B, T, H, heads, dm, scale, s)
#define ATX_D(D_)                                                                     \
    do {                                                                              \
        if (nt <= 4) ATX(4, D_, 8); else if (nt <= 8) ATX(8, D_, 8); else if (nt <= 13) ATX(13, D_, 8); else ATX(16, D_, 4); \
    } while (0)
        if (D == 32) ATX_D(32);
        else ATX_D(64);
#undef ATX_D
#undef ATX
    }
#define ATB(NT_, D_) return launch_att_bwd_f32<NT_, D_>(qkv, qkv_lo, dctx, dctx_lo, dqkv, dqkv_lo, fv, B, T, H, heads, dm, scale, s)
#define ATB_D(D_)                                                                     \
    do {                                                                              \
        if (nt <= 4) ATB(4, D_); else if (nt <= 8) ATB(8, D_); else if (nt <= 13) ATB(13, D_); else ATB(16, D_); \
    } while (0)
    if (D == 32) ATB_D(32);
    else if (D == 64) ATB_D(64);
    else ATB_D(128);
#undef ATB_D
#undef ATB
    return ADVH_EUNSUPPORTED;
}

ADVH_SPLIT_FLAG_SETTER(advh_split_flag_attention_bwd_ragged)
