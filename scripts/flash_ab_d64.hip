// flash_ab_d64.hip -- within-process A/B of the attn_flash_kernel forms at head dim 64 (SD-2.x: 5 heads at the 64x64 level, Lq 4096,
// 10 heads at 32x32, Lq 1024; kv slots [-1, 'first'] = 2 x Lq keys), interleaved rounds, TF/s priced at 4 Lq (2 Lkf) C per frame,
// uniform random operands (q as to_q produces it: no log2 fold at d = 64), outputs cross-checked against variant 0 (the old dispatch).
// Tuning tool, never part of the library (the product's choice lives in fz_attn_flash_dispatch).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffast-math -fno-finite-math-only -w -o build_tmp/flash_ab_d64 scripts/flash_ab_d64.hip
#define FZ_FLASH_NO_DISPATCH 1
#include "../fatezero_amd/csrc/attn_flash.hip"
#include <stdio.h>
#include <algorithm>
#include <vector>

typedef int (*LaunchFn)(const FzAttnSelfDesc&, const void*, const void*, const void*, void*, void*);
struct Variant {
    const char* name;
    LaunchFn fn;
};

int main(int argc, char** argv) {
    const Variant vars[] = {
        {"<64,W2,QB1> (dispatch before: every lq)", launch_flash<64, 2, 1>},
        {"<64,W2,QB2> two query blocks per wave   ", launch_flash<64, 2, 2>},
        {"<64,W4,QB1> four waves per SIMD         ", launch_flash<64, 4, 1>},
    };
    const int NV = sizeof(vars) / sizeof(vars[0]);
    const int D = 64;
    struct Shape { int F, H, L; };
    const Shape shapes[] = {{8, 5, 4096}, {16, 5, 4096}, {8, 10, 1024}, {16, 10, 1024}, {16, 20, 256}};
    for (const Shape& sh : shapes) {
        const int F = sh.F, H = sh.H, L = sh.L, C = H * D;
        FzAttnSelfDesc d = {};
        d.n_frames = F; d.frame0 = 0; d.clip_len = 8; d.heads = H; d.head_dim = D; d.lq = L; d.lkf = L; d.n_kv = 2;
        d.kv_abs[0] = 0; d.kv_val[0] = -1; d.kv_abs[1] = 1; d.kv_val[1] = 0;
        d.scale = 0.125f; d.mode = 0; d.q_log2_scaled = 0;
        d.q_frame_stride = (int64_t)L * 2 * C; d.q_row_stride = 2 * C;
        d.k_frame_stride = (int64_t)L * 2 * C; d.k_row_stride = 2 * C;
        d.vt_frame_stride = (int64_t)C * L; d.vt_chan_stride = L;
        d.o_frame_stride = (int64_t)L * C; d.o_row_stride = C;
        const size_t nqk = (size_t)F * L * 2 * C, nv = (size_t)F * C * L, no = (size_t)F * L * C;
        std::vector<_Float16> hqk(nqk), hv(nv);
        unsigned s = 12345;
        auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.0f * 2.0f - 1.0f; };
        for (size_t i = 0; i < nqk; ++i) hqk[i] = (_Float16)(rnd() * 1.5f);
        for (auto& x : hv) x = (_Float16)rnd();
        _Float16 *qk, *vt, *o[8];
        hipMalloc(&qk, nqk * 2); hipMalloc(&vt, nv * 2);
        for (int v = 0; v < NV; ++v) { hipMalloc(&o[v], no * 2); hipMemset(o[v], 0, no * 2); }
        hipMemcpy(qk, hqk.data(), nqk * 2, hipMemcpyHostToDevice);
        hipMemcpy(vt, hv.data(), nv * 2, hipMemcpyHostToDevice);
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        const int ROUNDS = 7, REP = 5;
        std::vector<std::vector<float>> ms(NV);
        int status = 0;
        for (int r = 0; r < ROUNDS; ++r)
            for (int v = 0; v < NV; ++v) {
                hipEventRecord(e0);
                for (int i = 0; i < REP; ++i) status |= vars[v].fn(d, qk, qk + C, vt, o[v], nullptr);
                hipEventRecord(e1);
                hipDeviceSynchronize();
                float t; hipEventElapsedTime(&t, e0, e1);
                if (r > 0) ms[v].push_back(t / REP);
            }
        if (status != 0) { printf("launch status %d\n", status); return 1; }
        const double flops = 4.0 * L * (2.0 * L) * C * F;
        std::vector<_Float16> ref(no), got(no);
        hipMemcpy(ref.data(), o[0], no * 2, hipMemcpyDeviceToHost);
        for (int v = 0; v < NV; ++v) {
            std::sort(ms[v].begin(), ms[v].end());
            hipMemcpy(got.data(), o[v], no * 2, hipMemcpyDeviceToHost);
            double maxd = 0, maxa = 0;
            for (size_t i = 0; i < no; ++i) {
                maxd = std::max(maxd, (double)fabsf((float)got[i] - (float)ref[i]));
                maxa = std::max(maxa, (double)fabsf((float)ref[i]));
            }
            const double med = ms[v][ms[v].size() / 2], mn = ms[v][0];
            printf("F=%2d H=%2d Lq=%4d %s median %.4f ms %7.1f TF/s | min %.4f ms %7.1f TF/s | max|o - o[0]| %.2e (max|o| %.3f)\n", F, H, L,
                   vars[v].name, med, flops / med / 1e9, mn, flops / mn / 1e9, maxd, maxa);
        }
        hipFree(qk); hipFree(vt);
        for (int v = 0; v < NV; ++v) hipFree(o[v]);
        fflush(stdout);
    }
    return 0;
}
