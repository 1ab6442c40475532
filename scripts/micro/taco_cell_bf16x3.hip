// The batched decoder's cell launches alone, fp32 (bg_kernel<2, 4, 4, 4, BG_EPI_CELL>, what the plain schedule runs above 64 rows)
// against the split-bf16 form (bgx_cell_kernel, tacotron_batched_bf16x3.h) in several launch shapes: the kernels of
// cookietts_amd/csrc/tacotron_decoder.hip compiled into this file, default decoder widths, random weights and state, whole launches
// timed with HIP events, arms alternated in one process.  Per cell (attention RNN 5120 x 2816, decoder RNN 3072 x 2560, second
// decoder RNN 3072 x 1536) and row count (128, 256): us per launch as the median over the repetitions, the spread (max - min), and
// L_inf of the new hidden state against the fp32 launch from the same state.  This was the go / no-go measurement of the mode
// (profiles/r18_00_taco_cell_bf16x3_ab.txt).  The library provides what the included source leaves undefined:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include scripts/micro/taco_cell_bf16x3.hip -o taco_cell_bf16x3 \
//         -L cookietts_amd -lcookietts_hip -Wl,-rpath,$PWD/cookietts_amd
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cookietts_amd/csrc/tacotron_decoder.hip"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
#define RC(x) do { int r_ = (x); if (r_) { printf("%s: rc %d: %s\n", #x, r_, ctts_last_error()); exit(1); } } while (0)

namespace {
using namespace ctts;

typedef int (*LaunchFn)(const BgArgs&, const float*, int, hipStream_t);
struct Arm { const char* name; LaunchFn fn; };

int launch_f32(const BgArgs& a, const float*, int nb, hipStream_t s) { return bg_launch_cell(a, nb, nullptr, nullptr, nullptr, a.batch, s, 0); }
template <int M, int N, int SS, int WV>
int launch_x3(const BgArgs& a, const float* planes, int nb, hipStream_t s) {
    return bgx_launch_shape<M, N, SS, WV>(bgx_args(a, planes), nb, nullptr, nullptr, nullptr, a.batch, s);
}

float* random_device(size_t n, float scale, unsigned seed) {
    std::vector<float> h(n);
    unsigned x = seed * 2654435761u + 12345u;
    for (size_t i = 0; i < n; ++i) { x = x * 1664525u + 1013904223u; h[i] = scale * ((x >> 8) * (1.0f / 8388608.0f) - 1.0f); }
    float* d;
    CK(hipMalloc(&d, n * 4));
    CK(hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice));
    return d;
}
}  // namespace

int main() {
    ctts_taco_decoder_config cfg{80, 1313, 512, 192, 1280, 768, 768, 256, 32, 31, 16};
    DecPlan p;
    RC(make_dec_plan(&cfg, p));
    if (!p.x3_ok) { printf("shape refused\n"); return 1; }
    const int T = 48;
    float* src = random_device((size_t)4 * 1280 * 1536 + 1313 * 512, 0.03f, 1);       // every weight pointer reads this buffer
    ctts_taco_decoder_weights wt{};
    wt.bottleneck_w = wt.memory_layer_w = wt.query_w = wt.v_w = wt.loc_conv_w = wt.loc_dense_w = wt.prenet_w1 = wt.prenet_w2 = src;
    wt.att_rnn = wt.dec_rnn = wt.dec2_rnn = ctts_lstm_weights{src, src + 777, src + 64, src + 128};
    wt.proj_w = wt.proj_b = wt.gate_w = wt.gate_b = src;
    float* blob;
    CK(hipMalloc(&blob, ctts_taco_decoder_packed_bf16x3_bytes(&cfg)));
    RC(ctts_taco_decoder_pack_bf16x3(&cfg, &wt, blob, nullptr));

    const Arm arms[] = {{"f32 <2,4,4,4>", launch_f32},
                        {"x3 <2,4,3,4>", launch_x3<2, 4, 3, 4>},
                        {"x3 <4,2,3,4>", launch_x3<4, 2, 3, 4>},
                        {"x3 <4,4,4,2>", launch_x3<4, 4, 4, 2>},
                        {"x3 <4,4,3,2>", launch_x3<4, 4, 3, 2>},
                        {"x3 <2,4,6,2>", launch_x3<2, 4, 6, 2>},
                        {"x3 <2,4,3,2>", launch_x3<2, 4, 3, 2>}};
    constexpr int NARMS = sizeof(arms) / sizeof(arms[0]);
    const int REPS = 7, PER = 20;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int batch : {128, 256}) {
        DecWs w;
        dec_carve(p, batch, T, nullptr, w);
        float* ws = random_device(w.total, 0.9f, 2);
        dec_carve(p, batch, T, ws, w);
        const int NB = ws_rows(p, batch), Pn = cfg.prenet_dim, Dm = cfg.memory_dim, Rd = cfg.decoder_rnn_dim, Ra = cfg.attention_rnn_dim;
        float *c0 = random_device((size_t)NB * Ra, 0.5f, 3), *cbuf, *hout[2];
        CK(hipMalloc(&cbuf, (size_t)NB * Ra * 4));
        for (auto& h : hout) { CK(hipMalloc(&h, (size_t)NB * Ra * 4)); CK(hipMemset(h, 0, (size_t)NB * Ra * 4)); }
        for (int cell = 0; cell < 3; ++cell) {
            BgArgs a{};
            const BgMat& m = cell == 0 ? p.bg_att : cell == 1 ? p.bg_dec : p.bg_d2;
            const size_t* lw = cell == 0 ? p.att : cell == 1 ? p.dec : p.d2;
            const float* planes = blob + (cell == 0 ? p.x3_att : cell == 1 ? p.x3_dec : p.x3_d2);
            a.W = blob + m.off; a.rows = m.rows; a.batch = batch;
            if (cell == 0) bg_set_x(a, m, w.prenet, Pn, w.ctx, Dm, w.dec_h[0], Rd, w.att_h[0], Ra);
            else if (cell == 1) bg_set_x(a, m, w.att_h[0], Ra, w.ctx, Dm, w.dec_h[0], Rd, nullptr, 0);
            else bg_set_x(a, m, w.dec_h[0], Rd, w.d2_h[0], Rd, nullptr, 0, nullptr, 0);
            a.bih = blob + lw[2]; a.bhh = blob + lw[3]; a.c = cbuf; a.H = cell == 0 ? Ra : Rd;
            const size_t nh = (size_t)batch * a.H;
            printf("cell %d (%d x %d), %d rows\n", cell, m.rows, m.nchunks * 16, batch);
            // the new hidden state of one launch from the same cell state, against the fp32 launch's
            std::vector<float> ref(nh), got(nh);
            for (int k = 0; k < NARMS; ++k) {
                CK(hipMemcpy(cbuf, c0, nh * 4, hipMemcpyDeviceToDevice));
                a.h_new = hout[k != 0];
                RC(arms[k].fn(a, planes, NB, nullptr));
                CK(hipDeviceSynchronize());
                CK(hipMemcpy(k ? got.data() : ref.data(), a.h_new, nh * 4, hipMemcpyDeviceToHost));
                double d = 0;
                if (k) for (size_t i = 0; i < nh; ++i) d = std::max(d, (double)std::fabs(got[i] - ref[i]));
                printf("  %-14s L_inf(h) vs f32 %.3g\n", arms[k].name, d);
            }
            a.h_new = hout[1];
            std::vector<float> us[NARMS];
            for (int rep = 0; rep < REPS + 1; ++rep)             // repetition 0 warms up
                for (int k = 0; k < NARMS; ++k) {
                    CK(hipEventRecord(e0, nullptr));
                    for (int i = 0; i < PER; ++i) RC(arms[k].fn(a, planes, NB, nullptr));
                    CK(hipEventRecord(e1, nullptr));
                    CK(hipEventSynchronize(e1));
                    float ms;
                    CK(hipEventElapsedTime(&ms, e0, e1));
                    if (rep) us[k].push_back(ms * 1000.f / PER);
                }
            for (int k = 0; k < NARMS; ++k) {
                std::sort(us[k].begin(), us[k].end());
                printf("  %-14s %8.2f us/launch  spread %.2f\n", arms[k].name, us[k][REPS / 2], us[k].back() - us[k].front());
            }
            fflush(stdout);
        }
        CK(hipFree(ws)); CK(hipFree(c0)); CK(hipFree(cbuf)); CK(hipFree(hout[0])); CK(hipFree(hout[1]));
    }
    return 0;
}
