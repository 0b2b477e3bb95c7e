// map8u_store_ab.hip -- same-process A/B of the two store paths of FZ_ATTN_CAPTURE8U (csrc/attn_self.hip): two key tiles of a kv slot
// leaving together as 128-byte row segments ("paired") against every tile leaving as 64-byte segments ("unpaired", the store path of
// FZ_ATTN_CAPTURE8), at the 32^2-level launch shape (1024 queries, two kv slots, 8 heads) at 8 and 16 frames, D = 40 and 80.  Each
// form is timed TWICE per round, back to back (A A B B): what two timings of the same form differ by is the spread a difference
// between the forms has to exceed.  The E5M2 and fp16 captures run beside them for scale.  The bytes both forms store are compared.
// Tuning tool, never part of the library.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffast-math -fno-finite-math-only -w -o build_tmp/map8u_store_ab scripts/map8u_store_ab.hip
#define FZ_SELF_NO_ENTRY 1
#include "../fatezero_amd/csrc/attn_self.hip"
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>

#define CK(x)                                                                      \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                    \
            printf("%s: %s\n", #x, hipGetErrorString(e_));                         \
            exit(2);                                                               \
        }                                                                          \
    } while (0)

// ABL bit 8 = the store path the library does NOT ship
constexpr int PAIRED = FZ_CAP8U_PAIRED ? 0 : 8, UNPAIRED = FZ_CAP8U_PAIRED ? 8 : 0;

template <int D, int MODE, int ABL>
static void run(const FzAttnSelfDesc& d, const half_t* q, const half_t* k, const half_t* vt, half_t* o, void* p) {
    const int nq = (d.lq + QBLK - 1) / QBLK;
    dim3 grid(nq * d.heads * d.n_frames), block(256);
    hipLaunchKernelGGL((attn_self_kernel<D, MODE, ABL>), grid, block, 0, 0, d, q, k, vt, o, (half_t*)p, (const float*)nullptr);
}

template <int D>
static int shape(int F) {
    const int H = 8, L = 1024, C = H * D;
    FzAttnSelfDesc d = {};
    d.n_frames = F; d.frame0 = 0; d.clip_len = F; d.heads = H; d.head_dim = D; d.lq = L; d.lkf = L; d.n_kv = 2;
    d.kv_abs[0] = 0; d.kv_val[0] = -1; d.kv_abs[1] = 1; d.kv_val[1] = 0;
    d.scale = 1.0f / sqrtf((float)D); d.q_log2_scaled = 0;
    d.q_frame_stride = (int64_t)L * 2 * C; d.q_row_stride = 2 * C;
    d.k_frame_stride = (int64_t)L * 2 * C; d.k_row_stride = 2 * C;
    d.vt_frame_stride = (int64_t)C * L; d.vt_chan_stride = L;
    d.o_frame_stride = (int64_t)L * C; d.o_row_stride = C;
    FzAttnSelfDesc d8 = d, d16 = d;  // p strides: bytes for the 8-bit modes, halves for fp16
    d8.p_row_stride = d16.p_row_stride = 2 * L;
    d8.p_head_stride = d16.p_head_stride = (int64_t)L * 2 * L;
    d8.p_frame_stride = d16.p_frame_stride = (int64_t)H * L * 2 * L;
    const size_t nqk = (size_t)F * L * 2 * C, nv = (size_t)F * C * L, no = (size_t)F * L * C, np = (size_t)F * H * L * 2 * L;
    std::vector<_Float16> hqk(nqk), hv(nv);
    unsigned s = 12345;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 65536.0f * 2.0f - 1.0f; };
    for (auto& x : hqk) x = (_Float16)(rnd() * 1.5f);
    for (auto& x : hv) x = (_Float16)rnd();
    _Float16 *qk, *vt, *o, *p16;
    uint8_t *pa, *pb;
    CK(hipMalloc(&qk, nqk * 2)); CK(hipMalloc(&vt, nv * 2)); CK(hipMalloc(&o, no * 2)); CK(hipMalloc(&p16, np * 2));
    CK(hipMalloc(&pa, np)); CK(hipMalloc(&pb, np));
    CK(hipMemcpy(qk, hqk.data(), nqk * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(vt, hv.data(), nv * 2, hipMemcpyHostToDevice));
    CK(hipMemset(pa, 0xA5, np)); CK(hipMemset(pb, 0x5A, np));
    // the two forms store the same bytes
    run<D, FZ_ATTN_CAPTURE8U, PAIRED>(d8, qk, qk + C, vt, o, pa);
    run<D, FZ_ATTN_CAPTURE8U, UNPAIRED>(d8, qk, qk + C, vt, o, pb);
    CK(hipDeviceSynchronize());
    CK(hipGetLastError());
    {
        std::vector<uint8_t> ha(np), hb(np);
        CK(hipMemcpy(ha.data(), pa, np, hipMemcpyDeviceToHost));
        CK(hipMemcpy(hb.data(), pb, np, hipMemcpyDeviceToHost));
        const bool same = memcmp(ha.data(), hb.data(), np) == 0;
        const uint8_t top = *std::max_element(ha.begin(), ha.end());
        printf("D %d, %d frames: paired and unpaired store %s bytes (largest byte 0x%02X)\n", D, F, same ? "the SAME" : "DIFFERENT", top);
        if (!same) return 1;
    }
    struct V { const char* name; void (*fn)(const FzAttnSelfDesc&, const half_t*, const half_t*, const half_t*, half_t*, void*); int p; };
    const V vars[] = {
        {"ue4m4 paired   #1", run<D, FZ_ATTN_CAPTURE8U, PAIRED>, 0},   {"ue4m4 paired   #2", run<D, FZ_ATTN_CAPTURE8U, PAIRED>, 0},
        {"ue4m4 unpaired #1", run<D, FZ_ATTN_CAPTURE8U, UNPAIRED>, 0}, {"ue4m4 unpaired #2", run<D, FZ_ATTN_CAPTURE8U, UNPAIRED>, 0},
        {"e5m2 (64-byte segments)", run<D, FZ_ATTN_CAPTURE8, 0>, 0},   {"fp16", run<D, FZ_ATTN_CAPTURE, 0>, 1},
    };
    const int NV = sizeof(vars) / sizeof(vars[0]);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int ROUNDS = 12, REP = 10;
    std::vector<std::vector<float>> ms(NV);
    for (int r = 0; r < ROUNDS; ++r)
        for (int v = 0; v < NV; ++v) {
            CK(hipEventRecord(e0));
            for (int i = 0; i < REP; ++i) vars[v].fn(vars[v].p ? d16 : d8, qk, qk + C, vt, o, vars[v].p ? (void*)p16 : (void*)pa);
            CK(hipEventRecord(e1));
            CK(hipDeviceSynchronize());
            float t;
            CK(hipEventElapsedTime(&t, e0, e1));
            if (r > 1) ms[v].push_back(t / REP);
        }
    double med[NV];
    for (int v = 0; v < NV; ++v) {
        std::sort(ms[v].begin(), ms[v].end());
        med[v] = ms[v][ms[v].size() / 2];
        printf("  %-26s median %.4f ms   min %.4f   max %.4f\n", vars[v].name, med[v], ms[v].front(), ms[v].back());
    }
    const double pa_ = 0.5 * (med[0] + med[1]), un_ = 0.5 * (med[2] + med[3]);
    const double spread = std::max(fabs(med[0] - med[1]), fabs(med[2] - med[3]));
    printf("  paired %.4f ms, unpaired %.4f ms: unpaired - paired = %+.4f ms (%.1f %%), same-form spread %.4f ms -> %s\n", pa_, un_, un_ - pa_,
           100.0 * (un_ - pa_) / un_, spread,
           un_ - pa_ > spread ? "paired is faster beyond the spread" : pa_ - un_ > spread ? "unpaired is faster beyond the spread" : "within the spread");
    CK(hipFree(qk)); CK(hipFree(vt)); CK(hipFree(o)); CK(hipFree(p16)); CK(hipFree(pa)); CK(hipFree(pb));
    return 0;
}

int main() {
    for (int F : {8, 16}) {
        if (shape<40>(F)) return 1;
        if (shape<80>(F)) return 1;
    }
    return 0;
}
