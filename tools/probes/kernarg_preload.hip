// Probe: does the firmware honour kernel-argument preloading (gfx940+: the leading kernel arguments arrive in user SGPRs at wave launch
// instead of being fetched by the wave's first s_load from the cold kernel-argument segment), and what is it worth per dependent launch?
//   hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-kernarg-preload-count=16 -o kernarg_preload         kernarg_preload.hip
//   hipcc --offload-arch=gfx950 -O3                                          -o kernarg_preload_noflag  kernarg_preload.hip     (control)
//   ./kernarg_preload && ./kernarg_preload_noflag
// Three kernels, each launched as a chain of CHAIN dependent one-workgroup launches on one stream (launch k reads buf[k], writes buf[k + 1]):
//   scalars  6 pointers + 2 ints as leading scalar parameters (14 dwords: preloaded when built with the flag, kernarg_preload_length 14)
//   struct   the same eight values inside one by-value struct (never preloaded, the form every kernel of the library has)
//   empty    no arguments read at all: the launch floor
// Each form runs twice: as it is ("tiny": the chain is then paced by how fast the host can submit, about 2.5 us per launch, and what a wave does at its
// head hides behind that), and with SPIN ticks of the 100 MHz clock spent behind the store ("busy", ~4 us per kernel: the host runs ahead, the launches
// queue up on the device as they do in the library's update loop, and the time per launch is what the device needs from one kernel to the next).
// With the flag, "scalars" against "struct" is the gain of preloading; without it the same pair is the control (both forms fetch their
// arguments with s_load, so they must agree), which separates preloading from any effect of the parameter layout.
// Every chain is timed REPS times (wall clock around CHAIN launches + one stream synchronise; hipEvent time beside it); the forms are
// alternated twice so that the spread between the two rounds of one form is the yardstick for the difference between forms.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int CHAIN = 200, REPS = 60, BUF = 256;   // BUF > CHAIN: launch k touches buf[k] and buf[k + 1] only

struct ChainArgs { const int* in; int* out; const int* a; const int* b; const int* c; const int* d; int k; int n; };

constexpr int SPIN = 400;   // "busy": 4 us at 100 MHz

template <int TICKS>
__device__ __forceinline__ void spin() {
    if (TICKS == 0) return;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < (unsigned long long)TICKS) __builtin_amdgcn_s_sleep(2);
}
template <int TICKS>
__device__ __forceinline__ void chain_body(const int* in, int* out, const int* a, const int* b, const int* c, const int* d, int k, int n) {
    if (threadIdx.x != 0 || k < 0 || k + 1 >= n) return;
    int v = in[k] + 1;
    if (v < 0) v += a[0] + b[0] + c[0] + d[0];     // never taken: keeps the other four pointers live
    out[k + 1] = v;
    spin<TICKS>();
}
template <int TICKS>
__global__ __launch_bounds__(64) void chain_scalars(const int* in, int* out, const int* a, const int* b, const int* c, const int* d, int k, int n) {
    chain_body<TICKS>(in, out, a, b, c, d, k, n);
}
template <int TICKS>
__global__ __launch_bounds__(64) void chain_struct(ChainArgs A) { chain_body<TICKS>(A.in, A.out, A.a, A.b, A.c, A.d, A.k, A.n); }
template <int TICKS>
__global__ __launch_bounds__(64) void chain_empty() { if (threadIdx.x == 0) spin<TICKS>(); }

enum Form { SCALARS, STRUCT, EMPTY };
static const char* const form_name[] = {"scalars", "struct ", "empty  "};

struct Timing { double wall_med, wall_min, ev_med; };

template <int TICKS>
static Timing run_form(Form f, int* buf, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    std::vector<double> wall, ev;
    for (int r = 0; r < REPS + 5; r++) {
        CK(hipMemsetAsync(buf, 0, BUF * sizeof(int), s));
        CK(hipStreamSynchronize(s));
        const auto t0 = std::chrono::steady_clock::now();
        CK(hipEventRecord(e0, s));
        for (int k = 0; k < CHAIN; k++) {
            if (f == SCALARS) hipLaunchKernelGGL(chain_scalars<TICKS>, dim3(1), dim3(64), 0, s, buf, buf, buf, buf, buf, buf, k, BUF);
            else if (f == STRUCT) { const ChainArgs A{buf, buf, buf, buf, buf, buf, k, BUF}; hipLaunchKernelGGL(chain_struct<TICKS>, dim3(1), dim3(64), 0, s, A); }
            else hipLaunchKernelGGL(chain_empty<TICKS>, dim3(1), dim3(64), 0, s);
        }
        CK(hipEventRecord(e1, s));
        CK(hipStreamSynchronize(s));
        const auto t1 = std::chrono::steady_clock::now();
        CK(hipGetLastError());
        float ms = 0.0f;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (f != EMPTY) {                          // the arguments arrived: the chain counted to CHAIN
            int last = -1;
            CK(hipMemcpy(&last, buf + CHAIN, sizeof(int), hipMemcpyDeviceToHost));
            if (last != CHAIN) { fprintf(stderr, "%s: chain ended at %d, expected %d\n", form_name[f], last, CHAIN); exit(2); }
        }
        if (r < 5) continue;                       // warm-up
        wall.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count() / CHAIN);
        ev.push_back(ms * 1e3 / CHAIN);
    }
    std::sort(wall.begin(), wall.end());
    std::sort(ev.begin(), ev.end());
    return {wall[wall.size() / 2], wall[0], ev[ev.size() / 2]};
}

int main() {
    int* buf;
    hipStream_t s;
    hipEvent_t e0, e1;
    CK(hipMalloc(&buf, BUF * sizeof(int)));
    CK(hipStreamCreate(&s));
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    printf("kernarg_preload: %d dependent launches per chain, %d chains per line, us per launch\n", CHAIN, REPS);
    printf("round kernel form     wall_median  wall_min  event_median\n");
    for (int round = 0; round < 2; round++)
        for (int busy = 0; busy < 2; busy++)
            for (Form f : {SCALARS, STRUCT, EMPTY}) {
                const Timing t = busy ? run_form<SPIN>(f, buf, s, e0, e1) : run_form<0>(f, buf, s, e0, e1);
                printf("%d     %s   %s  %10.3f %9.3f %13.3f\n", round, busy ? "busy" : "tiny", form_name[f], t.wall_med, t.wall_min, t.ev_med);
            }
    CK(hipFree(buf));
    return 0;
}
