// attn_temporal.hip -- temporal attention over the F frames of every (batch, pixel, head): the un-patched
// diffusers CrossAttention.forward applied on '(b d) f c' (attention.py:327-337 of the reference).
//
// Up to 64 frames the sequence length is the clip length (8..32 in the reference's configs), so this is a bandwidth problem, not an
// MFMA one (longer clips take attn_temporal_long_kernel, up to 256 frames, and attn_temporal_stream_kernel, up to
// FZ_TEMPORAL_MAX_FRAMES, further down, which are MFMA ones): q, k, v stay
// in their native token-major layout [(b f)][token][channel] (no '(b f) d c -> (b d) f c' rearrange is ever
// materialised); one thread owns one (token, head, query frame), the F key/value rows of its pixel are shared
// through L1 by the F threads of that pixel, and scores live in LDS.
#include "fz_rt.h"
#include "../../include/fatezero_hip.h"
#include <stdlib.h>

#define TMAXF 64                                 // the one-thread-per-query-frame kernels below serve clips up to here ...
#define TLONG_MAXF 256                           // ... attn_temporal_long_kernel (matrix pipe, whole score rows in registers) up to here ...
#define TSTREAM_MAXF FZ_TEMPORAL_MAX_FRAMES      // ... attn_temporal_stream_kernel (matrix pipe, keys walked in chunks) the longer ones
#define TTHREADS 256

struct TemporalArgs {
    const half_t *q, *k, *v;
    half_t* o;
    int batch, F, Fq, tokens, heads, dh;  // F key/value frames, Fq query frames per batch element
    int64_t in_stride, q_stride, out_stride;
    float scale;
    int tok_per_block;
};

FZ_KERNEL void __launch_bounds__(TTHREADS) attn_temporal_kernel(TemporalArgs a) {
    FZ_DYN_SMEM(raw);
    float* S = reinterpret_cast<float*>(raw);  // [TTHREADS][F]
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int tok0 = blockIdx.x * a.tok_per_block;
    const int items = a.tok_per_block * a.heads * a.Fq;
    const int nvec = a.dh >> 3;
    float* myS = S + tid * a.F;
    for (int w = tid; w < items; w += TTHREADS) {
        const int h = w % a.heads;
        const int tl = (w / a.heads) % a.tok_per_block;
        const int i = w / (a.heads * a.tok_per_block);
        const int tok = tok0 + tl;
        if (tok >= a.tokens) continue;
        const int64_t col = (int64_t)h * a.dh;
        const half_t* qrow = a.q + ((int64_t)(b * a.Fq + i) * a.tokens + tok) * a.q_stride + col;
        // pass 1: scores
        float mx = -1e30f;
        for (int j = 0; j < a.F; ++j) {
            const half_t* krow = a.k + ((int64_t)(b * a.F + j) * a.tokens + tok) * a.in_stride + col;
            float acc = 0.0f;
            for (int c = 0; c < nvec; ++c) {
                const half8_t qv = fz_ld_h8(qrow + 8 * c), kv = fz_ld_h8(krow + 8 * c);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc += (float)qv[e] * (float)kv[e];
            }
            acc *= a.scale;
            myS[j] = acc;
            mx = fmaxf(mx, acc);
        }
        float sum = 0.0f;
        for (int j = 0; j < a.F; ++j) {
            const float e = __builtin_expf(myS[j] - mx);
            myS[j] = e;
            sum += e;
        }
        const float inv = 1.0f / sum;
        for (int j = 0; j < a.F; ++j) myS[j] = (float)(half_t)(myS[j] * inv);  // P is cast to fp16 before P.V
        // pass 2: O = P V
        half_t* orow = a.o + ((int64_t)(b * a.Fq + i) * a.tokens + tok) * a.out_stride + col;
        for (int c = 0; c < nvec; ++c) {
            float acc[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
            for (int j = 0; j < a.F; ++j) {
                const half8_t vv = fz_ld_h8(a.v + ((int64_t)(b * a.F + j) * a.tokens + tok) * a.in_stride + col + 8 * c);
                const float pj = myS[j];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += pj * (float)vv[e];
            }
            half8_t ov;
#pragma unroll
            for (int e = 0; e < 8; ++e) ov[e] = (half_t)acc[e];
            fz_st_h8(orow + 8 * c, ov);
        }
    }
}

// LDS-staged form (the default whenever the K/V rows of a token group fit): the F key rows and F value rows of
// `tok_per_block` tokens are copied global -> LDS once, with every lane moving 16 contiguous bytes of a 2C-byte row,
// instead of being re-read through L1 by each of the F query frames with an 80..320-byte lane stride.
//   * FT > 0: the clip length is a compile-time constant -- scores and probabilities live in registers (no LDS round trip),
//     every loop unrolls; FT == 0: any clip length, scores in LDS.
//   * the rows of odd tokens are stored rotated by 8 chunks (128 B): a 16-lane group of a ds_read_b128 spans two tokens whose
//     rows are a multiple of 256 B apart, which without the rotation is a 2-way bank conflict on every read.
//   * no padding: 4 tokens x 8 frames x (K + V) of the 320-channel level are exactly 40 KB, four workgroups per CU, and the
//     1024 workgroups of a 64x64 frame batch are one full wave of the chip (with the score buffer in LDS three fitted:
//     1.33 rounds).
template <int FT>
FZ_KERNEL void __launch_bounds__(TTHREADS) attn_temporal_lds_kernel(TemporalArgs a) {
    FZ_DYN_SMEM(raw);
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int tok0 = blockIdx.x * a.tok_per_block;
    const int F = FT > 0 ? FT : a.F;
    const int C = a.heads * a.dh, cvec = C >> 3;
    half_t* Ks = reinterpret_cast<half_t*>(raw);                  // [tok_per_block][F][C]
    half_t* Vs = Ks + (size_t)a.tok_per_block * F * C;            // same
    float* S = reinterpret_cast<float*>(Vs + (size_t)a.tok_per_block * F * C);  // FT == 0: [TTHREADS][F]
    const int rows = a.tok_per_block * F;
    const int rot = cvec > 8 ? 8 : 0;  // rotation of odd tokens' rows, in 16-byte chunks
    for (int id = tid; id < rows * cvec; id += TTHREADS) {
        const int row = id / cvec, cv = id % cvec;
        const int tl = row / F, j = row % F;
        int tok = tok0 + tl;
        tok = tok < a.tokens ? tok : a.tokens - 1;
        const int64_t g = ((int64_t)(b * F + j) * a.tokens + tok) * a.in_stride + cv * 8;
        int dc = cv + ((tl & 1) ? rot : 0);
        dc = dc >= cvec ? dc - cvec : dc;
        fz_st_h8(Ks + (size_t)row * C + dc * 8, fz_ld_h8(a.k + g));
        fz_st_h8(Vs + (size_t)row * C + dc * 8, fz_ld_h8(a.v + g));
    }
    __syncthreads();
    const int items = a.tok_per_block * a.heads * a.Fq;
    const int nvec = a.dh >> 3;
    float* myS = S + tid * F;
    for (int w = tid; w < items; w += TTHREADS) {
        const int h = w % a.heads;
        const int tl = (w / a.heads) % a.tok_per_block;
        const int i = w / (a.heads * a.tok_per_block);
        const int tok = tok0 + tl;
        if (tok >= a.tokens) continue;
        const int col = h * a.dh;
        const half_t* qrow = a.q + ((int64_t)(b * a.Fq + i) * a.tokens + tok) * a.q_stride + col;
        const half_t* kt = Ks + (size_t)tl * F * C;
        const half_t* vtok = Vs + (size_t)tl * F * C;
        const int c0 = (col >> 3) + ((tl & 1) ? rot : 0);  // first (rotated) chunk of this head inside a row
        half_t* orow = a.o + ((int64_t)(b * a.Fq + i) * a.tokens + tok) * a.out_stride + col;
        if (FT > 0) {
            constexpr int FR = FT > 0 ? FT : 1;
            float s[FR];
#pragma unroll
            for (int j = 0; j < FR; ++j) s[j] = 0.0f;
            for (int c = 0; c < nvec; ++c) {
                int cc = c0 + c;
                cc = cc >= cvec ? cc - cvec : cc;
                const half8_t qv = fz_ld_h8(qrow + 8 * c);
#pragma unroll
                for (int j = 0; j < FR; ++j) {
                    const half8_t kv = fz_ld_h8(kt + (size_t)j * C + cc * 8);
#pragma unroll
                    for (int e = 0; e < 8; ++e) s[j] += (float)qv[e] * (float)kv[e];
                }
            }
            float mx = -1e30f;
#pragma unroll
            for (int j = 0; j < FR; ++j) {
                s[j] *= a.scale;
                mx = fmaxf(mx, s[j]);
            }
            float sum = 0.0f;
#pragma unroll
            for (int j = 0; j < FR; ++j) {
                s[j] = __builtin_expf(s[j] - mx);
                sum += s[j];
            }
            const float inv = 1.0f / sum;
#pragma unroll
            for (int j = 0; j < FR; ++j) s[j] = (float)(half_t)(s[j] * inv);  // P is cast to fp16 before P.V
            for (int c = 0; c < nvec; ++c) {
                int cc = c0 + c;
                cc = cc >= cvec ? cc - cvec : cc;
                float acc[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
#pragma unroll
                for (int j = 0; j < FR; ++j) {
                    const half8_t vv = fz_ld_h8(vtok + (size_t)j * C + cc * 8);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += s[j] * (float)vv[e];
                }
                half8_t ov;
#pragma unroll
                for (int e = 0; e < 8; ++e) ov[e] = (half_t)acc[e];
                fz_st_h8(orow + 8 * c, ov);
            }
        } else {
            float mx = -1e30f;
            for (int j = 0; j < F; ++j) {
                float acc = 0.0f;
                for (int c = 0; c < nvec; ++c) {
                    int cc = c0 + c;
                    cc = cc >= cvec ? cc - cvec : cc;
                    const half8_t qv = fz_ld_h8(qrow + 8 * c), kv = fz_ld_h8(kt + (size_t)j * C + cc * 8);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc += (float)qv[e] * (float)kv[e];
                }
                acc *= a.scale;
                myS[j] = acc;
                mx = fmaxf(mx, acc);
            }
            float sum = 0.0f;
            for (int j = 0; j < F; ++j) {
                const float e = __builtin_expf(myS[j] - mx);
                myS[j] = e;
                sum += e;
            }
            const float inv = 1.0f / sum;
            for (int j = 0; j < F; ++j) myS[j] = (float)(half_t)(myS[j] * inv);  // P is cast to fp16 before P.V
            for (int c = 0; c < nvec; ++c) {
                int cc = c0 + c;
                cc = cc >= cvec ? cc - cvec : cc;
                float acc[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
                for (int j = 0; j < F; ++j) {
                    const half8_t vv = fz_ld_h8(vtok + (size_t)j * C + cc * 8);
                    const float pj = myS[j];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += pj * (float)vv[e];
                }
                half8_t ov;
#pragma unroll
                for (int e = 0; e < 8; ++e) ov[e] = (half_t)acc[e];
                fz_st_h8(orow + 8 * c, ov);
            }
        }
    }
}

// Long clips (kv_frames or q_frames > 64): per (token, head) this is a small dense attention, F x F x d, and the F^2 work of the
// one-thread-per-query-frame kernels above would sit on the vector ALUs -- so both products go to the matrix pipe
// (v_mfma_f32_32x32x16_f16) in the TRANSPOSED form, which needs no register transpose between them:
//   S^T = K Q^T   A = K tile [32 keys][16 ch], B = Q^T [16 ch][32 queries]: both fragments are 16 contiguous bytes of a global row.
//                 C: lane (i, hi) holds, for query i, keys 32t + 8g + 4hi + r of tile t in register 4g + r (g, r = 0..3).
//   softmax       over the keys of a query = over the lane's NT x 16 registers and the lane pair (l, l ^ 32).  The WHOLE row is in
//                 registers (NT <= 8 tiles x 16 fp32), so it is the exact two-pass softmax of the reference: P is normalised, THEN
//                 rounded to fp16, then multiplied -- an online softmax could only round the un-normalised P.  That register file of
//                 scores is what ends this kernel at 8 x 32 = 256 frames (attn_temporal_stream_kernel below takes over there).
//   O^T = V^T P^T B = P^T [16 keys][32 queries] is the C fragment above as it lies (registers 8kc..8kc+7 of tile t -> half8), i.e.
//                 contraction slot (kc, hi, e) of tile t is key 32t + 16kc + 8(e >> 2) + 4hi + (e & 3): bits 2 and 3 of the key's
//                 offset inside its group of 16 are swapped against the natural order.  A = V^T [32 ch][16 keys] has to supply
//                 the same keys in the same slots: V is staged once per workgroup into LDS TRANSPOSED, Vt[head][ch][key position],
//                 with that swap applied to the position, so an A fragment is one 16-byte LDS read.
//                 C: lane (i, hi) holds, for query i, channels 32ct + 8g + 4hi + r: four 8-byte stores per channel tile.
// One workgroup = one (batch element, token, group of `hg` heads); its 4 waves share the staged V and split the (head, 32-query
// tile) items.  Frames beyond the clip (F % 32 != 0) and channels beyond head_dim (head_dim % 32 != 0) are never read: their
// fragments are zero, the scores of padded keys are masked before the softmax, and the padded key positions of Vt are zero-filled
// (P is exactly 0 there; 0 x stale LDS could still be NaN).
struct TemporalLongArgs {
    const half_t *q, *k, *v;
    half_t* o;
    int F, Fq, tokens, heads, dh;
    int hg, ngroups, ldv;  // heads per workgroup, workgroups per token, halves between channel rows of Vt (32 NT + 8)
    int64_t in_stride, q_stride, out_stride;
    float scale;
};

FZ_DEVICE int tlong_key_pos(int key) { return (key & ~12) | ((key & 4) << 1) | ((key & 8) >> 1); }

template <int NT>
FZ_KERNEL void __launch_bounds__(TTHREADS) attn_temporal_long_kernel(TemporalLongArgs a) {
    FZ_DYN_SMEM(raw);
    half_t* Vt = reinterpret_cast<half_t*>(raw);  // [hg][dh][ldv]
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int tok = blockIdx.x / a.ngroups;
    const int h0 = (blockIdx.x % a.ngroups) * a.hg;
    const int F = a.F, dh = a.dh, ldv = a.ldv;
    const int nvec = dh >> 3;
    // ---- stage V of the group's heads, transposed: lanes walk the keys (adjacent 2-byte LDS columns), then chunks, then heads
    for (int id = tid; id < a.hg * nvec * (NT * 32); id += TTHREADS) {
        const int key = id % (NT * 32), cv = (id / (NT * 32)) % nvec, hl = id / (NT * 32 * nvec);
        half8_t vv = fz_zero_h8();
        if (key < F) vv = fz_ld_h8(a.v + ((int64_t)(b * F + key) * a.tokens + tok) * a.in_stride + (h0 + hl) * dh + cv * 8);
        half_t* dst = Vt + ((size_t)hl * dh + cv * 8) * ldv + tlong_key_pos(key);
#pragma unroll
        for (int e = 0; e < 8; ++e) dst[(size_t)e * ldv] = vv[e];
    }
    __syncthreads();
    const int lane = tid & 63, wave = fz_uniform(tid >> 6);
    const int i = lane & 31, hi = lane >> 5;
    const int nq = (a.Fq + 31) >> 5;
    const int64_t kv_frame = (int64_t)a.tokens * a.in_stride;  // halves between the same token of consecutive frames
    for (int item = wave; item < a.hg * nq; item += TTHREADS / 64) {
        const int hl = item / nq, qt = item % nq;
        const int col = (h0 + hl) * dh;
        const int qf = qt * 32 + i;
        const bool qok = qf < a.Fq;
        const half_t* qrow = a.q + ((int64_t)(b * a.Fq + (qok ? qf : 0)) * a.tokens + tok) * a.q_stride + col;
        const half_t* krow = a.k + ((int64_t)b * F * a.tokens + tok) * a.in_stride + col;  // frame 0 of this batch element
        // ---- S^T = K Q^T
        f32x16 s[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) s[t] = fz_zero_f16v();
        for (int c0 = 0; c0 < dh; c0 += 16) {
            const int ch = c0 + 8 * hi;
            const bool chok = ch < dh;
            const half8_t qfrag = (qok && chok) ? fz_ld_h8(qrow + ch) : fz_zero_h8();
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int key = 32 * t + i;
                const half8_t kfrag = (key < F && chok) ? fz_ld_h8(krow + key * kv_frame + ch) : fz_zero_h8();
                s[t] = fz_mfma_32x32x16_f16(kfrag, qfrag, s[t]);
            }
        }
        // ---- exact softmax over the keys of query i
        float mx = -1e30f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * t + 8 * (r >> 2) + 4 * hi + (r & 3);
                const float x = key < F ? s[t][r] * a.scale : -1e30f;
                s[t][r] = x;
                mx = fmaxf(mx, x);
            }
        mx = fz_pair_max32(mx);
        float sum = 0.0f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * t + 8 * (r >> 2) + 4 * hi + (r & 3);
                const float e = key < F ? __builtin_expf(s[t][r] - mx) : 0.0f;
                s[t][r] = e;
                sum += e;
            }
        sum += fz_shfl_xor(sum, 32);
        const float inv = 1.0f / sum;
        half8_t p[NT][2];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) p[t][r >> 3][r & 7] = (half_t)(s[t][r] * inv);  // P is cast to fp16 before P.V
        // ---- O^T = V^T P^T, one 32-channel tile at a time
        const half_t* vh = Vt + (size_t)hl * dh * ldv;
        half_t* orow = a.o + ((int64_t)(b * a.Fq + (qok ? qf : 0)) * a.tokens + tok) * a.out_stride + col;
        for (int c0 = 0; c0 < dh; c0 += 32) {
            const bool chok = c0 + i < dh;
            const half_t* vrow = vh + (size_t)(chok ? c0 + i : 0) * ldv + 8 * hi;
            f32x16 acc = fz_zero_f16v();
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int kc = 0; kc < 2; ++kc) {
                    const half8_t vfrag = chok ? fz_ld_h8(vrow + 32 * t + 16 * kc) : fz_zero_h8();
                    acc = fz_mfma_32x32x16_f16(vfrag, p[t][kc], acc);
                }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch = c0 + 8 * g + 4 * hi;
                if (qok && ch < dh) {
                    half4_t ov;
#pragma unroll
                    for (int r = 0; r < 4; ++r) ov[r] = (half_t)acc[4 * g + r];
                    *reinterpret_cast<half4_t*>(orow + ch) = ov;
                }
            }
        }
    }
}

// heads per workgroup of the long-clip kernel: the largest divisor of `heads` whose transposed V fits 64 KB (two workgroups per CU and
// no opt-in attribute); a single head beyond that (head_dim 160 from 193 frames) takes the opt-in path, 84.5 KB at the very most
static int tlong_launch(const TemporalLongArgs& a0, int batch, void* stream) {
    TemporalLongArgs a = a0;
    const int nt = (a.F + 31) / 32;  // (q_frames > 64 >= kv_frames is legal too: the key tiles follow kv_frames alone)
    a.ldv = nt * 32 + 8;
    const size_t per_head = (size_t)a.dh * a.ldv * sizeof(half_t);
    a.hg = 1;
    for (int g = a.heads; g >= 1; --g)
        if (a.heads % g == 0 && g * per_head <= 64 * 1024) {
            a.hg = g;
            break;
        }
    a.ngroups = a.heads / a.hg;
    const size_t lds = a.hg * per_head;
    if (lds > 160 * 1024 || (int64_t)a.tokens * a.ngroups > 0x7fffffff || batch > 65535) return FZ_ERR_UNSUPPORTED;
    dim3 grid((unsigned)(a.tokens * a.ngroups), batch), block(TTHREADS);
    auto launch = [&](auto kern) -> int { return FZ_LAUNCH_LDS(kern, grid, block, lds, stream, a); };
    switch (nt) {
        case 1: return launch(attn_temporal_long_kernel<1>);
        case 2: return launch(attn_temporal_long_kernel<2>);
        case 3: return launch(attn_temporal_long_kernel<3>);
        case 4: return launch(attn_temporal_long_kernel<4>);
        case 5: return launch(attn_temporal_long_kernel<5>);
        case 6: return launch(attn_temporal_long_kernel<6>);
        case 7: return launch(attn_temporal_long_kernel<7>);
        case 8: return launch(attn_temporal_long_kernel<8>);
    }
    return FZ_ERR_BAD_ARG;
}

// Clips beyond 256 frames (kv_frames or q_frames > TLONG_MAXF): the same two transposed MFMA products, but nothing in the kernel's
// register or LDS footprint grows with the clip -- the keys are walked in CHUNKS of TSTREAM_CHUNK = 256 frames by a run-time loop.
// The numeric contract is unchanged (P = half(exp(s - m) * (1 / l)) with m and l over ALL keys in fp32, O accumulated in fp32 and
// rounded once), which an online softmax cannot meet (it could only round the un-normalised P and rescale O), so the keys are
// walked TWICE:
//   sweep 1   S^T tile by tile (32 keys x 32 queries, K fragments straight from global rows as above): every lane keeps a running
//             maximum and a rescaled running sum over the keys it holds; the lane pair (l, l ^ 32) is combined once at the end.
//             No LDS, no barrier.
//   sweep 2   per chunk: V of the chunk is staged transposed (tlong_key_pos swap, zero-filled beyond the clip) between two
//             barriers, then every score tile of the chunk is RECOMPUTED by the same function (the same MFMA chain; the compiler may
//             contract the scale into the subtraction of m on one side only: at most an fp32 ulp of a score, five orders of
//             magnitude below the fp16 rounding of P), turned into the final fp16 P with the m and 1 / l of sweep 1, and
//             multiplied into O^T.
//             The O^T accumulators (16 fp32 per 32-channel tile) stay in registers across the chunks.
// Q K^T twice is the cheap side of the trade: per (token, head) the whole problem is F x F x d, and the alternative -- keeping F
// scores per query somewhere -- is what tied the long kernel's footprint to the clip length.
// One workgroup = one (batch element, token, group of HG heads, group of four 32-query tiles): wave w owns query tile 4 qg + w for
// all HG heads (a wave whose tile lies beyond q_frames only helps staging).  The Q fragments of the wave's tile are loaded once and
// kept in registers for both sweeps.  HG * CT <= 5 accumulator tiles (CT = channel tiles of a head): 80 fp32 at head_dim 160.
#define TSTREAM_CHUNK 256
#define TSTREAM_LDV (TSTREAM_CHUNK + 8)  // halves between channel rows of Vt: 132 dwords, rows 4 banks apart
struct TemporalStreamArgs {
    const half_t *q, *k, *v;
    half_t* o;
    int F, Fq, tokens, heads, dh;
    int ngroups, nqg;  // head groups per token, groups of four query tiles per (token, head group)
    int64_t in_stride, q_stride, out_stride;
    float scale;
};

// scores of key tile `t` (32 keys) against the wave's 32 queries, scaled, keys beyond the clip at -1e30: lane (i, hi) holds for
// query i the keys 32t + 8g + 4hi + r in register 4g + r.  kcol: column `8 hi` of the head in frame 0's row of this token.
template <int CT>
FZ_DEVICE f32x16 tstream_scores(const half_t* kcol, int64_t kv_frame, int t, int i, int hi, int F, int dh, float scale,
                                const half8_t (&qfr)[2 * CT]) {
    f32x16 s = fz_zero_f16v();
    const int key = 32 * t + i;
    const half_t* krow = kcol + (key < F ? key : 0) * kv_frame;
#pragma unroll
    for (int cs = 0; cs < 2 * CT; ++cs)
        if (16 * cs < dh) {
            const half8_t kfrag = (key < F && 16 * cs + 8 * hi < dh) ? fz_ld_h8(krow + 16 * cs) : fz_zero_h8();
            s = fz_mfma_32x32x16_f16(kfrag, qfr[cs], s);
        }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int kr = 32 * t + 8 * (r >> 2) + 4 * hi + (r & 3);
        s[r] = kr < F ? s[r] * scale : -1e30f;
    }
    return s;
}

template <int HG, int CT>
FZ_KERNEL void __launch_bounds__(TTHREADS) attn_temporal_stream_kernel(TemporalStreamArgs a) {
    FZ_DYN_SMEM(raw);
    half_t* Vt = reinterpret_cast<half_t*>(raw);  // [HG][dh][TSTREAM_LDV]
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    int bx = blockIdx.x;
    const int qg = bx % a.nqg;
    bx /= a.nqg;
    const int h0 = (bx % a.ngroups) * HG;
    const int tok = bx / a.ngroups;
    const int F = a.F, dh = a.dh;
    const int nvec = dh >> 3;
    const int lane = tid & 63, wave = fz_uniform(tid >> 6);
    const int i = lane & 31, hi = lane >> 5;
    const int ntiles = (F + 31) >> 5, nchunks = (F + TSTREAM_CHUNK - 1) / TSTREAM_CHUNK;
    const int qt = qg * (TTHREADS / 64) + wave;
    const bool active = qt < ((a.Fq + 31) >> 5);  // wave-uniform
    const int qf = qt * 32 + i;
    const bool qok = active && qf < a.Fq;
    const int64_t kv_frame = (int64_t)a.tokens * a.in_stride;  // halves between the same token of consecutive frames
    const int64_t qo_row = ((int64_t)b * a.Fq + (qok ? qf : 0)) * a.tokens + tok;
    const half_t* qrow = a.q + qo_row * a.q_stride + h0 * dh;
    const half_t* kcol = a.k + ((int64_t)b * F * a.tokens + tok) * a.in_stride + h0 * dh + 8 * hi;  // frame 0 of this batch element
    const half_t* vcol = a.v + ((int64_t)b * F * a.tokens + tok) * a.in_stride + h0 * dh;
    half8_t qfr[HG][2 * CT];
#pragma unroll
    for (int hl = 0; hl < HG; ++hl)
#pragma unroll
        for (int cs = 0; cs < 2 * CT; ++cs) {
            const int ch = 16 * cs + 8 * hi;
            qfr[hl][cs] = (qok && ch < dh) ? fz_ld_h8(qrow + hl * dh + ch) : fz_zero_h8();
        }
    // ---- sweep 1: m and 1 / l of every query over ALL keys
    float mx[HG], inv[HG];
#pragma unroll
    for (int hl = 0; hl < HG; ++hl) mx[hl] = 0.0f, inv[hl] = 0.0f;
    if (active) {
#pragma unroll
        for (int hl = 0; hl < HG; ++hl) {
            float m = -1e30f, l = 0.0f;
            for (int t = 0; t < ntiles; ++t) {
                const f32x16 s = tstream_scores<CT>(kcol + hl * dh, kv_frame, t, i, hi, F, dh, a.scale, qfr[hl]);
                float mn = m;
#pragma unroll
                for (int r = 0; r < 16; ++r) mn = fmaxf(mn, s[r]);
                float ts = 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kr = 32 * t + 8 * (r >> 2) + 4 * hi + (r & 3);
                    ts += kr < F ? __builtin_expf(s[r] - mn) : 0.0f;
                }
                l = l * __builtin_expf(m - mn) + ts;
                m = mn;
            }
            const float mall = fz_pair_max32(m);
            l *= __builtin_expf(m - mall);
            l += fz_shfl_xor(l, 32);
            mx[hl] = mall;
            inv[hl] = 1.0f / l;
        }
    }
    // ---- sweep 2: chunk by chunk, V staged transposed, scores recomputed, O^T accumulated
    f32x16 acc[HG][CT];
#pragma unroll
    for (int hl = 0; hl < HG; ++hl)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[hl][ct] = fz_zero_f16v();
    for (int c = 0; c < nchunks; ++c) {
        const int k0 = c * TSTREAM_CHUNK;
        const int ntc = ntiles - c * (TSTREAM_CHUNK / 32) < TSTREAM_CHUNK / 32 ? ntiles - c * (TSTREAM_CHUNK / 32) : TSTREAM_CHUNK / 32;
        const int ckeys = ntc * 32;  // key positions of this chunk (whole tiles; beyond the clip zero-filled)
        if (c) __syncthreads();      // every wave has read the previous chunk's V
        for (int id = tid; id < HG * nvec * ckeys; id += TTHREADS) {
            const int key = id % ckeys, cv = (id / ckeys) % nvec, hl = id / (ckeys * nvec);
            half8_t vv = fz_zero_h8();
            if (k0 + key < F) vv = fz_ld_h8(vcol + (k0 + key) * kv_frame + hl * dh + cv * 8);
            half_t* dst = Vt + ((size_t)hl * dh + cv * 8) * TSTREAM_LDV + tlong_key_pos(key);
#pragma unroll
            for (int e = 0; e < 8; ++e) dst[(size_t)e * TSTREAM_LDV] = vv[e];
        }
        __syncthreads();
        if (!active) continue;
#pragma unroll
        for (int hl = 0; hl < HG; ++hl)
            for (int t = 0; t < ntc; ++t) {
                const int tg = c * (TSTREAM_CHUNK / 32) + t;
                const f32x16 s = tstream_scores<CT>(kcol + hl * dh, kv_frame, tg, i, hi, F, dh, a.scale, qfr[hl]);
                half8_t p[2];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int kr = 32 * tg + 8 * (r >> 2) + 4 * hi + (r & 3);
                    const float e = kr < F ? __builtin_expf(s[r] - mx[hl]) : 0.0f;
                    p[r >> 3][r & 7] = (half_t)(e * inv[hl]);  // P is normalised, THEN cast to fp16, then multiplied
                }
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
                    if (32 * ct < dh) {
                        const bool chok = 32 * ct + i < dh;
                        const half_t* vrow = Vt + ((size_t)hl * dh + (chok ? 32 * ct + i : 0)) * TSTREAM_LDV + 32 * t + 8 * hi;
#pragma unroll
                        for (int kc = 0; kc < 2; ++kc) {
                            const half8_t vfrag = chok ? fz_ld_h8(vrow + 16 * kc) : fz_zero_h8();
                            acc[hl][ct] = fz_mfma_32x32x16_f16(vfrag, p[kc], acc[hl][ct]);
                        }
                    }
            }
    }
    if (!qok) return;
    half_t* orow = a.o + qo_row * a.out_stride + h0 * dh;
#pragma unroll
    for (int hl = 0; hl < HG; ++hl)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch = 32 * ct + 8 * g + 4 * hi;
                if (ch < dh) {
                    half4_t ov;
#pragma unroll
                    for (int r = 0; r < 4; ++r) ov[r] = (half_t)acc[hl][ct][4 * g + r];
                    *reinterpret_cast<half4_t*>(orow + hl * dh + ch) = ov;
                }
            }
}

// heads per workgroup of the streaming kernel: the long kernel's rule (the largest divisor of `heads` whose transposed V chunk fits
// 64 KB; a single head beyond that -- head_dim 128..160 -- takes the opt-in path, 82.5 KB at the most) with one more bound: the
// group's O^T accumulators, HG x CT tiles of 16 fp32, are capped at 5 tiles.  head_dim > 160 is not served by this form.
static int tstream_launch(const TemporalStreamArgs& a0, int batch, void* stream) {
    TemporalStreamArgs a = a0;
    const int ct = (a.dh + 31) / 32;
    if (ct > 5) return FZ_ERR_UNSUPPORTED;
    const size_t per_head = (size_t)a.dh * TSTREAM_LDV * sizeof(half_t);
    int hg = 1;
    for (int g = a.heads; g >= 1; --g)
        if (a.heads % g == 0 && g * per_head <= 64 * 1024 && g * ct <= 5) {
            hg = g;
            break;
        }
    a.ngroups = a.heads / hg;
    a.nqg = ((a.Fq + 31) / 32 + TTHREADS / 64 - 1) / (TTHREADS / 64);
    const size_t lds = hg * per_head;
    if (lds > 160 * 1024 || (int64_t)a.tokens * a.ngroups * a.nqg > 0x7fffffff || batch > 65535) return FZ_ERR_UNSUPPORTED;
    dim3 grid((unsigned)(a.tokens * a.ngroups * a.nqg), batch), block(TTHREADS);
    auto launch = [&](auto kern) -> int { return FZ_LAUNCH_LDS(kern, grid, block, lds, stream, a); };
    switch (hg * 8 + ct) {
        case 1 * 8 + 1: return launch(attn_temporal_stream_kernel<1, 1>);
        case 1 * 8 + 2: return launch(attn_temporal_stream_kernel<1, 2>);
        case 1 * 8 + 3: return launch(attn_temporal_stream_kernel<1, 3>);
        case 1 * 8 + 4: return launch(attn_temporal_stream_kernel<1, 4>);
        case 1 * 8 + 5: return launch(attn_temporal_stream_kernel<1, 5>);
        case 2 * 8 + 1: return launch(attn_temporal_stream_kernel<2, 1>);
        case 2 * 8 + 2: return launch(attn_temporal_stream_kernel<2, 2>);
        case 3 * 8 + 1: return launch(attn_temporal_stream_kernel<3, 1>);
        case 4 * 8 + 1: return launch(attn_temporal_stream_kernel<4, 1>);
        case 5 * 8 + 1: return launch(attn_temporal_stream_kernel<5, 1>);
    }
    return FZ_ERR_BAD_ARG;
}

extern "C" int fz_attn_temporal_ex(const void* q, const void* k, const void* v, void* o, int batch, int q_frames,
                                   int kv_frames, int tokens, int heads, int head_dim, int64_t q_row_stride,
                                   int64_t kv_row_stride, int64_t o_row_stride, float scale, void* stream) {
    if (!q || !k || !v || !o || batch <= 0 || q_frames <= 0 || kv_frames <= 0 || kv_frames > TSTREAM_MAXF ||
        q_frames > TSTREAM_MAXF || tokens <= 0 || heads <= 0 || head_dim <= 0)
        return FZ_ERR_BAD_ARG;
    if ((head_dim & 7) || (q_row_stride & 7) || (kv_row_stride & 7) || (o_row_stride & 7)) return FZ_ERR_BAD_ARG;
    if (kv_frames > TLONG_MAXF || q_frames > TLONG_MAXF) {  // beyond 256 frames: the streaming kernel.  Up to there nothing below has changed.
        TemporalStreamArgs t;
        t.q = (const half_t*)q; t.k = (const half_t*)k; t.v = (const half_t*)v; t.o = (half_t*)o;
        t.F = kv_frames; t.Fq = q_frames; t.tokens = tokens; t.heads = heads; t.dh = head_dim;
        t.ngroups = t.nqg = 0;
        t.in_stride = kv_row_stride; t.q_stride = q_row_stride; t.out_stride = o_row_stride; t.scale = scale;
        return tstream_launch(t, batch, stream);
    }
    if (kv_frames > TMAXF || q_frames > TMAXF) {  // long clips: the matrix-pipe kernel.  Up to TMAXF nothing below has changed.
        TemporalLongArgs l;
        l.q = (const half_t*)q; l.k = (const half_t*)k; l.v = (const half_t*)v; l.o = (half_t*)o;
        l.F = kv_frames; l.Fq = q_frames; l.tokens = tokens; l.heads = heads; l.dh = head_dim;
        l.hg = l.ngroups = l.ldv = 0;
        l.in_stride = kv_row_stride; l.q_stride = q_row_stride; l.out_stride = o_row_stride; l.scale = scale;
        return tlong_launch(l, batch, stream);
    }
    TemporalArgs a;
    a.q = (const half_t*)q; a.k = (const half_t*)k; a.v = (const half_t*)v; a.o = (half_t*)o;
    a.batch = batch; a.F = kv_frames; a.Fq = q_frames; a.tokens = tokens; a.heads = heads; a.dh = head_dim;
    a.in_stride = kv_row_stride; a.q_stride = q_row_stride; a.out_stride = o_row_stride; a.scale = scale;
    int tpb = TTHREADS / (heads * q_frames);
    if (tpb < 1) tpb = 1;
    // clip lengths with a register-resident instantiation: 8 (the judged config), 16, and since round 3 24 / 32 (BASELINE cfg4 / cfg5:
    // at 32 frames the generic kernel was 16.6 % of the cfg5-shaped job)
    const bool fixed = kv_frames == 8 || kv_frames == 16 || kv_frames == 24 || kv_frames == 32;
    const size_t score_bytes_lds = fixed ? 0 : (size_t)TTHREADS * kv_frames * sizeof(float);
    const size_t score_bytes = (size_t)TTHREADS * kv_frames * sizeof(float);
    const size_t kv_bytes_per_token = (size_t)2 * kv_frames * heads * head_dim * sizeof(half_t);
    int tpb_lds = tpb;
    while (tpb_lds > 1 && tpb_lds * kv_bytes_per_token + score_bytes_lds > 40 * 1024) tpb_lds >>= 1;  // 40 KB: four per CU
    const size_t lds = tpb_lds * kv_bytes_per_token + score_bytes_lds;
    if (lds <= 160 * 1024) {  // (one token of a 32-frame clip at 1280 channels is exactly 160 KB)
        a.tok_per_block = tpb_lds;
        dim3 grid((tokens + tpb_lds - 1) / tpb_lds, batch), block(TTHREADS);
        auto launch = [&](auto kern) -> int { return FZ_LAUNCH_LDS(kern, grid, block, lds, stream, a); };
        switch (fixed ? kv_frames : 0) {
            case 8: return launch(attn_temporal_lds_kernel<8>);
            case 16: return launch(attn_temporal_lds_kernel<16>);
            case 24: return launch(attn_temporal_lds_kernel<24>);
            case 32: return launch(attn_temporal_lds_kernel<32>);
            default: return launch(attn_temporal_lds_kernel<0>);
        }
    }
    a.tok_per_block = tpb;
    dim3 grid((tokens + tpb - 1) / tpb, batch), block(TTHREADS);
    FZ_LAUNCH(attn_temporal_kernel, grid, block, score_bytes, stream, a);
    return fz_last_launch_status();
}

extern "C" int fz_attn_temporal(const void* q, const void* k, const void* v, void* o, int batch, int clip_len,
                                int tokens, int heads, int head_dim, int64_t qkv_row_stride, int64_t o_row_stride,
                                float scale, void* stream) {
    return fz_attn_temporal_ex(q, k, v, o, batch, clip_len, clip_len, tokens, heads, head_dim, qkv_row_stride,
                               qkv_row_stride, o_row_stride, scale, stream);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Windowed temporal attention (fz_attn_temporal_win): query frame f -- an ABSOLUTE index among the kv_frames, q_frame0 + its row --
// attends the key/value frames j with |j - f| <= W, cut at the clip's ends (nothing is padded: frame 0 attends W + 1 frames).  The
// numeric contract is the one of every kernel above: scores in fp32, the exact softmax over the attended keys, P normalised, THEN
// rounded to fp16, O accumulated in fp32 and rounded once.  A window that covers the clip (W >= kv_frames - 1) never gets here: the
// entry point hands it to fz_attn_temporal_ex.  Nothing above this line is touched by the windowed form.
//
// Up to TMAXF key/value frames: attn_temporal_kernel with loop bounds -- one thread per (token, head, query frame), the at most
// 2 W + 1 scores of its band in LDS.
struct TemporalWinArgs {
    const half_t *q, *k, *v;
    half_t* o;
    int batch, F, Fq, q0, W, ns, tokens, heads, dh;  // ns: score slots per thread, min(2 W + 1, F)
    int64_t in_stride, q_stride, out_stride;
    float scale;
    int tok_per_block;
};

FZ_KERNEL void __launch_bounds__(TTHREADS) attn_temporal_win_kernel(TemporalWinArgs a) {
    FZ_DYN_SMEM(raw);
    float* S = reinterpret_cast<float*>(raw);  // [TTHREADS][ns]
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int tok0 = blockIdx.x * a.tok_per_block;
    const int items = a.tok_per_block * a.heads * a.Fq;
    const int nvec = a.dh >> 3;
    float* myS = S + tid * a.ns;
    for (int w = tid; w < items; w += TTHREADS) {
        const int h = w % a.heads;
        const int tl = (w / a.heads) % a.tok_per_block;
        const int i = w / (a.heads * a.tok_per_block);
        const int tok = tok0 + tl;
        if (tok >= a.tokens) continue;
        const int f = a.q0 + i;  // absolute frame of this query
        const int j0 = f - a.W > 0 ? f - a.W : 0;
        const int j1 = f + a.W < a.F - 1 ? f + a.W : a.F - 1;  // the band [j0, j1]: never empty (q0 + Fq <= F), at most ns frames
        const int64_t col = (int64_t)h * a.dh;
        const half_t* qrow = a.q + ((int64_t)(b * a.Fq + i) * a.tokens + tok) * a.q_stride + col;
        float mx = -1e30f;
        for (int j = j0; j <= j1; ++j) {
            const half_t* krow = a.k + ((int64_t)(b * a.F + j) * a.tokens + tok) * a.in_stride + col;
            float acc = 0.0f;
            for (int c = 0; c < nvec; ++c) {
                const half8_t qv = fz_ld_h8(qrow + 8 * c), kv = fz_ld_h8(krow + 8 * c);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc += (float)qv[e] * (float)kv[e];
            }
            acc *= a.scale;
            myS[j - j0] = acc;
            mx = fmaxf(mx, acc);
        }
        float sum = 0.0f;
        for (int j = j0; j <= j1; ++j) {
            const float e = __builtin_expf(myS[j - j0] - mx);
            myS[j - j0] = e;
            sum += e;
        }
        const float inv = 1.0f / sum;
        for (int j = j0; j <= j1; ++j) myS[j - j0] = (float)(half_t)(myS[j - j0] * inv);  // P is cast to fp16 before P.V
        half_t* orow = a.o + ((int64_t)(b * a.Fq + i) * a.tokens + tok) * a.out_stride + col;
        for (int c = 0; c < nvec; ++c) {
            float acc[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
            for (int j = j0; j <= j1; ++j) {
                const half8_t vv = fz_ld_h8(a.v + ((int64_t)(b * a.F + j) * a.tokens + tok) * a.in_stride + col + 8 * c);
                const float pj = myS[j - j0];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += pj * (float)vv[e];
            }
            half8_t ov;
#pragma unroll
            for (int e = 0; e < 8; ++e) ov[e] = (half_t)acc[e];
            fz_st_h8(orow + 8 * c, ov);
        }
    }
}

// Beyond TMAXF key/value frames: the band kernel.  The two transposed MFMA products of attn_temporal_long_kernel (S^T = K Q^T with
// whole score rows in registers, the exact two-pass softmax, O^T = V^T P^T with P^T the C fragment as it lies), but a 32-query tile
// contracts only the key tiles that overlap its band:
//   tile arithmetic   the wave's queries are the absolute frames a0 .. a0 + 31 (a0 = q_frame0 + 32 qt), their keys lie in
//                     [a0 - W, a0 + 31 + W] cut at the clip's ends.  Key tiles are ALIGNED TO ABSOLUTE MULTIPLES OF 32 FRAMES (first tile
//                     t0 = max(a0 - W, 0) / 32), so a key always sits in the same fragment slot whatever q_frame0 and whichever other
//                     queries share the launch; a span of 32 + 2 W frames touches at most NT = ceil((32 + 2 W) / 32) + 1 aligned tiles:
//                     2 at W = 0, 3 up to W = 16, 8 at W = 96 = FZ_TEMPORAL_MAX_WINDOW (the 8 x 16 fp32 score registers
//                     attn_temporal_long_kernel<8> holds without scratch).  Tiles of the NT that lie wholly beyond the band or the clip are
//                     skipped (wave-uniform).
//   mask              key j counts for query f iff |j - f| <= W and j < F; every other score is -1e30 before the softmax and its P is
//                     exactly 0.  The sum over a row runs in a FIXED order with re-association off: masked slots add an exact 0, so a
//                     query's l -- and with it every bit of its output -- does not depend on where its tile's first key tile lies.  That
//                     is what makes a frame-sharded launch bit-equal to the same rows of the whole-clip launch.
//   V                 is never staged for the clip, nor for the band: per (32-channel tile, key tile) the wave stages ONE 32 x 32
//                     block transposed (tlong_key_pos swap, zero-filled beyond the clip and beyond head_dim) into its OWN 2.5 KB of
//                     LDS, reads the two A fragments back and moves on.  Wave-private: no workgroup barrier anywhere in the kernel, and
//                     10 KB of LDS per workgroup whatever the clip, the window and the head dimension.
// Work follows F (2 W + 1): Fq / 32 query tiles x NT key tiles.  One workgroup = one (batch element, token, group of `hg` heads,
// four consecutive 32-query tiles): wave w owns tile 4 qg + w and walks the group's heads; the waves of a workgroup share their
// overlapping K / V rows (and the heads of a token their cache lines) through L1.
#define TBAND_LDV 40  // halves between channel rows of a wave's Vt block: 20 dwords, 16 lanes of a ds_read_b128 on 16 distinct bank quads
struct TemporalBandArgs {
    const half_t *q, *k, *v;
    half_t* o;
    int F, Fq, q0, W, tokens, heads, dh;
    int hg, ngroups, nqg;  // heads per workgroup, head groups per token, groups of four query tiles
    int64_t in_stride, q_stride, out_stride;
    float scale;
};

template <int NT>
FZ_KERNEL void __launch_bounds__(TTHREADS) attn_temporal_band_kernel(TemporalBandArgs a) {
    FZ_DYN_SMEM(raw);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = fz_uniform(tid >> 6);
    half_t* Vt = reinterpret_cast<half_t*>(raw) + wave * (32 * TBAND_LDV);  // [32 channels][TBAND_LDV], this wave's own
    const int b = blockIdx.y;
    int bx = blockIdx.x;
    const int qg = bx % a.nqg;
    bx /= a.nqg;
    const int h0 = (bx % a.ngroups) * a.hg;
    const int tok = bx / a.ngroups;
    const int qt = qg * (TTHREADS / 64) + wave;
    if (qt * 32 >= a.Fq) return;  // wave-uniform; the kernel has no workgroup barrier
    const int F = a.F, dh = a.dh, W = a.W;
    const int i = lane & 31, hi = lane >> 5;
    const int qf = qt * 32 + i;
    const bool qok = qf < a.Fq;
    const int qabs = a.q0 + (qok ? qf : a.Fq - 1);  // (a lane beyond q_frames mirrors the last query: a non-empty band, nothing stored)
    const int a0 = a.q0 + qt * 32;                  // absolute frame of the tile's first query
    const int alast = (qt * 32 + 31 < a.Fq ? qt * 32 + 31 : a.Fq - 1) + a.q0;
    const int t0 = (a0 - W > 0 ? a0 - W : 0) >> 5;                 // first (aligned) key tile of the band
    const int kend = alast + W + 1 < F ? alast + W + 1 : F;        // keys >= kend: beyond the band of every query here, or the clip
    const int klo = qabs - W, khi = qabs + W < F - 1 ? qabs + W : F - 1;  // this lane's band [klo, khi] (klo may be negative)
    const int64_t kv_frame = (int64_t)a.tokens * a.in_stride;      // halves between the same token of consecutive frames
    const int64_t qo_row = ((int64_t)b * a.Fq + (qok ? qf : 0)) * a.tokens + tok;
    const half_t* kbase = a.k + ((int64_t)b * F * a.tokens + tok) * a.in_stride;  // frame 0 of this batch element
    const half_t* vbase = a.v + ((int64_t)b * F * a.tokens + tok) * a.in_stride;
    for (int hl = 0; hl < a.hg; ++hl) {
        const int col = (h0 + hl) * dh;
        const half_t* qrow = a.q + qo_row * a.q_stride + col;
        // ---- S^T = K Q^T over the band's key tiles
        f32x16 s[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) s[t] = fz_zero_f16v();
        for (int c0 = 0; c0 < dh; c0 += 16) {
            const int ch = c0 + 8 * hi;
            const bool chok = ch < dh;
            const half8_t qfrag = (qok && chok) ? fz_ld_h8(qrow + ch) : fz_zero_h8();
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (32 * (t0 + t) >= kend) continue;  // wave-uniform
                const int key = 32 * (t0 + t) + i;
                const half8_t kfrag = (key < kend && chok) ? fz_ld_h8(kbase + key * kv_frame + col + ch) : fz_zero_h8();
                s[t] = fz_mfma_32x32x16_f16(kfrag, qfrag, s[t]);
            }
        }
        // ---- exact softmax over the band of query qabs
        float mx = -1e30f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = 32 * (t0 + t) + 8 * (r >> 2) + 4 * hi + (r & 3);
                const float x = (key >= klo && key <= khi) ? s[t][r] * a.scale : -1e30f;
                s[t][r] = x;
                mx = fmaxf(mx, x);
            }
        mx = fz_pair_max32(mx);
        float sum = 0.0f;
        {
#ifndef FZ_EMU
#pragma clang fp reassociate(off)
#endif
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    // (a masked slot holds -1e30 and mx is a real score -- the band is never empty: its exp is exactly 0, and the
                    // 16 NT lane masks of the first sweep need not be kept alive for this one)
                    const float e = __builtin_expf(s[t][r] - mx);
                    s[t][r] = e;
                    sum = sum + e;
                }
        }
        sum += fz_shfl_xor(sum, 32);
        const float inv = 1.0f / sum;
        half8_t p[NT][2];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) p[t][r >> 3][r & 7] = (half_t)(s[t][r] * inv);  // P is cast to fp16 before P.V
        // ---- O^T = V^T P^T, one 32-channel tile at a time, V block by block through the wave's own LDS
        half_t* orow = a.o + qo_row * a.out_stride + col;
        for (int c0 = 0; c0 < dh; c0 += 32) {
            f32x16 acc = fz_zero_f16v();
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (32 * (t0 + t) >= kend) continue;  // wave-uniform
                const int key = 32 * (t0 + t) + i;
#pragma unroll
                for (int it = 0; it < 2; ++it) {
                    const int cv = 2 * it + hi;  // 8-channel chunk of the 32-channel tile
                    half8_t vv = fz_zero_h8();
                    if (key < F && c0 + 8 * cv < dh) vv = fz_ld_h8(vbase + key * kv_frame + col + c0 + 8 * cv);
                    half_t* dst = Vt + (8 * cv) * TBAND_LDV + tlong_key_pos(i);
#pragma unroll
                    for (int e = 0; e < 8; ++e) dst[e * TBAND_LDV] = vv[e];
                }
                fz_wave_lds_sync();  // the block is written by the wave's lanes and read back by other lanes of the same wave
#pragma unroll
                for (int kc = 0; kc < 2; ++kc) {
                    const half8_t vfrag = fz_ld_h8(Vt + i * TBAND_LDV + 8 * hi + 16 * kc);
                    acc = fz_mfma_32x32x16_f16(vfrag, p[t][kc], acc);
                }
                fz_wave_lds_sync();  // ... and is overwritten by the next block only after these reads
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch = c0 + 8 * g + 4 * hi;
                if (qok && ch < dh) {
                    half4_t ov;
#pragma unroll
                    for (int r = 0; r < 4; ++r) ov[r] = (half_t)acc[4 * g + r];
                    *reinterpret_cast<half4_t*>(orow + ch) = ov;
                }
            }
        }
    }
}

static_assert(FZ_TEMPORAL_MAX_WINDOW == 96, "the band kernel's instantiations end at 8 key tiles: ceil((32 + 2 W) / 32) + 1 <= 8");

// heads per workgroup of the band kernel: all of them (the heads of a token share cache lines), halved while the grid would leave
// most of the chip idle -- a head's result does not depend on the grouping
static int tband_launch(const TemporalBandArgs& a0, int batch, void* stream) {
    TemporalBandArgs a = a0;
    const int nt = (32 + 2 * a.W + 31) / 32 + 1;
    a.nqg = ((a.Fq + 31) / 32 + TTHREADS / 64 - 1) / (TTHREADS / 64);
    a.hg = a.heads;
    while (a.hg % 2 == 0 && (int64_t)a.tokens * (a.heads / a.hg) * a.nqg * batch < 2048) a.hg /= 2;
    a.ngroups = a.heads / a.hg;
    if ((int64_t)a.tokens * a.ngroups * a.nqg > 0x7fffffff || batch > 65535) return FZ_ERR_UNSUPPORTED;
    const size_t lds = (size_t)(TTHREADS / 64) * 32 * TBAND_LDV * sizeof(half_t);
    dim3 grid((unsigned)(a.tokens * a.ngroups * a.nqg), batch), block(TTHREADS);
    auto launch = [&](auto kern) -> int { return FZ_LAUNCH_LDS(kern, grid, block, lds, stream, a); };
    switch (nt) {
        case 2: return launch(attn_temporal_band_kernel<2>);
        case 3: return launch(attn_temporal_band_kernel<3>);
        case 4: return launch(attn_temporal_band_kernel<4>);
        case 5: return launch(attn_temporal_band_kernel<5>);
        case 6: return launch(attn_temporal_band_kernel<6>);
        case 7: return launch(attn_temporal_band_kernel<7>);
        case 8: return launch(attn_temporal_band_kernel<8>);
    }
    return FZ_ERR_BAD_ARG;
}

extern "C" int fz_attn_temporal_win(const void* q, const void* k, const void* v, void* o, int batch, int q_frames, int kv_frames,
                                    int q_frame0, int window, int tokens, int heads, int head_dim, int64_t q_row_stride,
                                    int64_t kv_row_stride, int64_t o_row_stride, float scale, void* stream) {
    if (!q || !k || !v || !o || batch <= 0 || q_frames <= 0 || kv_frames <= 0 || kv_frames > TSTREAM_MAXF || window < 0 ||
        q_frame0 < 0 || (int64_t)q_frame0 + q_frames > kv_frames || tokens <= 0 || heads <= 0 || head_dim <= 0)
        return FZ_ERR_BAD_ARG;
    if ((head_dim & 7) || (q_row_stride & 7) || (kv_row_stride & 7) || (o_row_stride & 7)) return FZ_ERR_BAD_ARG;
    if (window >= kv_frames - 1)  // the window covers the clip for every query: today's launch, bit for bit
        return fz_attn_temporal_ex(q, k, v, o, batch, q_frames, kv_frames, tokens, heads, head_dim, q_row_stride, kv_row_stride,
                                   o_row_stride, scale, stream);
    if (kv_frames > TMAXF) {
        if (window > FZ_TEMPORAL_MAX_WINDOW) return FZ_ERR_UNSUPPORTED;
        TemporalBandArgs t;
        t.q = (const half_t*)q; t.k = (const half_t*)k; t.v = (const half_t*)v; t.o = (half_t*)o;
        t.F = kv_frames; t.Fq = q_frames; t.q0 = q_frame0; t.W = window; t.tokens = tokens; t.heads = heads; t.dh = head_dim;
        t.hg = t.ngroups = t.nqg = 0;
        t.in_stride = kv_row_stride; t.q_stride = q_row_stride; t.out_stride = o_row_stride; t.scale = scale;
        return tband_launch(t, batch, stream);
    }
    TemporalWinArgs a;
    a.q = (const half_t*)q; a.k = (const half_t*)k; a.v = (const half_t*)v; a.o = (half_t*)o;
    a.batch = batch; a.F = kv_frames; a.Fq = q_frames; a.q0 = q_frame0; a.W = window; a.tokens = tokens; a.heads = heads; a.dh = head_dim;
    a.ns = 2 * window + 1 < kv_frames ? 2 * window + 1 : kv_frames;
    a.in_stride = kv_row_stride; a.q_stride = q_row_stride; a.out_stride = o_row_stride; a.scale = scale;
    int tpb = TTHREADS / (heads * q_frames);
    if (tpb < 1) tpb = 1;
    a.tok_per_block = tpb;
    if (batch > 65535) return FZ_ERR_UNSUPPORTED;
    dim3 grid((tokens + tpb - 1) / tpb, batch), block(TTHREADS);
    return FZ_LAUNCH_LDS(attn_temporal_win_kernel, grid, block, (size_t)TTHREADS * a.ns * sizeof(float), stream, a);
}
