// flash_kv_slots.hip -- what more kv slots cost in attn_flash_kernel<40,2,2> on the 64x64 SD level (d = 40, Lq = Lkf = 4096, 8 heads): 8 INTERIOR
// frames (4..11) of a 16-frame clip, so that every slot of every frame is a distinct source frame, under lists of 2, 5 and 8 entries.
// Interleaved rounds in one process; TF/s priced over the key tiles actually contracted (4 Lq (n_kv Lkf) C per frame).  Uniform random
// [-1.5, 1.5) operands.  Measuring tool, never part of the library.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffast-math -fno-finite-math-only -w -o build_tmp/flash_kv_slots scripts/flash_kv_slots.hip
#define FZ_FLASH_NO_DISPATCH 1
#include "../fatezero_amd/csrc/attn_flash.hip"
#include <stdio.h>
#include <algorithm>
#include <vector>

struct List {
    const char* name;
    int n_kv;
    int kv_abs[FZ_MAX_KV_SLOTS], kv_val[FZ_MAX_KV_SLOTS];
};

int main() {
    const int CLIP = 16, F0 = 4, F = 8, H = 8, L = 4096, D = 40, C = H * D;
    const List lists[] = {
        {"[-1, 'last']                              2 slots", 2, {0, 1}, {-1, CLIP - 1}},
        {"[-2, -1, 'first', 1, 2]                   5 slots", 5, {0, 0, 1, 0, 0}, {-2, -1, 0, 1, 2}},
        {"['first', -3, -2, -1, 1, 2, 3, 'last']    8 slots", 8, {1, 0, 0, 0, 0, 0, 0, 1}, {0, -3, -2, -1, 1, 2, 3, CLIP - 1}},
    };
    const int NL = sizeof(lists) / sizeof(lists[0]);
    const size_t nqk = (size_t)CLIP * L * 2 * C, nv = (size_t)CLIP * C * L, no = (size_t)CLIP * L * C;
    std::vector<_Float16> hqk(nqk), hv(nv);
    unsigned s = 12345;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.0f * 2.0f - 1.0f; };
    for (size_t i = 0; i < nqk; ++i) {  // q is in the log2 domain: a 1.5-scaled operand times scale * log2(e)
        const bool is_q = (i % (2 * C)) < (size_t)C;
        hqk[i] = (_Float16)(rnd() * 1.5f * (is_q ? 0.158113883f * 1.44269504f : 1.0f));
    }
    for (auto& x : hv) x = (_Float16)rnd();
    _Float16 *qk, *vt, *o;
    if (hipMalloc(&qk, nqk * 2) != hipSuccess || hipMalloc(&vt, nv * 2) != hipSuccess || hipMalloc(&o, no * 2) != hipSuccess) return 1;
    hipMemcpy(qk, hqk.data(), nqk * 2, hipMemcpyHostToDevice);
    hipMemcpy(vt, hv.data(), nv * 2, hipMemcpyHostToDevice);
    hipMemset(o, 0, no * 2);
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    const int ROUNDS = 7, REP = 5;
    std::vector<std::vector<float>> ms(NL);
    for (int r = 0; r < ROUNDS; ++r)
        for (int v = 0; v < NL; ++v) {
            FzAttnSelfDesc d = {};
            d.n_frames = F; d.frame0 = F0; d.clip_len = CLIP; d.heads = H; d.head_dim = D; d.lq = L; d.lkf = L; d.n_kv = lists[v].n_kv;
            for (int j = 0; j < lists[v].n_kv; ++j) { d.kv_abs[j] = lists[v].kv_abs[j]; d.kv_val[j] = lists[v].kv_val[j]; }
            d.scale = 0.158113883f; d.mode = 0; d.q_log2_scaled = 1;
            d.q_frame_stride = (int64_t)L * 2 * C; d.q_row_stride = 2 * C;
            d.k_frame_stride = (int64_t)L * 2 * C; d.k_row_stride = 2 * C;
            d.vt_frame_stride = (int64_t)C * L; d.vt_chan_stride = L;
            d.o_frame_stride = (int64_t)L * C; d.o_row_stride = C;
            for (int j = 1; j < d.n_kv; ++j)  // the point of the frame range: no two slots of a frame coincide
                for (int f = F0; f < F0 + F; ++f)
                    for (int i = 0; i < j; ++i)
                        if (fl_kv_source(d, 0, f, i) == fl_kv_source(d, 0, f, j)) { printf("slots %d and %d of frame %d coincide\n", i, j, f); return 1; }
            hipEventRecord(e0);
            for (int i = 0; i < REP; ++i)
                if (launch_flash<40, 2, 2, true, 2>(d, qk, qk + C, vt, o, nullptr) != 0) { printf("launch failed\n"); return 1; }
            hipEventRecord(e1);
            if (hipDeviceSynchronize() != hipSuccess) { printf("device error\n"); return 1; }
            float t;
            hipEventElapsedTime(&t, e0, e1);
            if (r > 0) ms[v].push_back(t / REP);
        }
    for (int v = 0; v < NL; ++v) {
        std::sort(ms[v].begin(), ms[v].end());
        const double flops = 4.0 * L * ((double)lists[v].n_kv * L) * C * F;
        const double med = ms[v][ms[v].size() / 2], mn = ms[v][0];
        printf("F=%d frames %d..%d of %d  %-52s median %.4f ms %7.1f TF/s | min %.4f ms %7.1f TF/s | ms per slot %.4f\n", F, F0, F0 + F - 1, CLIP,
               lists[v].name, med, flops / med / 1e9, mn, flops / mn / 1e9, med / lists[v].n_kv);
    }
    hipFree(qk); hipFree(vt); hipFree(o);
    return 0;
}
