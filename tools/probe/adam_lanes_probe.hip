// Probe: the Adam (+ EMA) element update of k_adam_sched (csrc/qk_opt.hip) with 4-byte lanes against 16-byte lanes, same grid cap, on
// buffers of the flat parameter count of TimitQCNN(10, 32); 1000 back-to-back launches per form, three rounds.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probe/adam_lanes_probe.hip -o tools/probe/adam_lanes_probe.bin
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

__device__ __forceinline__ void elem(float &p, float g, float &m, float &v, float d, float &e, float unscale, float coef, float lr_t, float omd, bool ema)
{
    float gi = g * unscale;
    gi = fmaf(d, p, gi);
    gi *= coef;
    const float mi = 0.9f * m + (1.f - 0.9f) * gi;
    const float vi = 0.999f * v + (1.f - 0.999f) * gi * gi;
    m = mi; v = vi;
    const float pn = p - lr_t * mi / (sqrtf(vi) + 1e-7f);
    p = pn;
    if (ema) e = e + omd * (pn - e);
}

template <bool EMA>
__global__ void __launch_bounds__(256) k4(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, const float *__restrict__ d, float *__restrict__ e, size_t n, float lr_t, float omd)
{
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    for (; i < n; i += stride) {
        float pp = p[i], mm = m[i], vv = v[i], ee = EMA ? e[i] : 0.f;
        elem(pp, g[i], mm, vv, d[i], ee, 0.5f, 0.75f, lr_t, omd, EMA);
        p[i] = pp; m[i] = mm; v[i] = vv;
        if (EMA) e[i] = ee;
    }
}

template <bool EMA>
__global__ void __launch_bounds__(256) k16(float4 *__restrict__ p, const float4 *__restrict__ g, float4 *__restrict__ m, float4 *__restrict__ v, const float4 *__restrict__ d, float4 *__restrict__ e, size_t n4, float lr_t, float omd)
{
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    for (; i < n4; i += stride) {
        float4 pp = p[i], mm = m[i], vv = v[i], gg = g[i], dd = d[i], ee = EMA ? e[i] : make_float4(0, 0, 0, 0);
        elem(pp.x, gg.x, mm.x, vv.x, dd.x, ee.x, 0.5f, 0.75f, lr_t, omd, EMA);
        elem(pp.y, gg.y, mm.y, vv.y, dd.y, ee.y, 0.5f, 0.75f, lr_t, omd, EMA);
        elem(pp.z, gg.z, mm.z, vv.z, dd.z, ee.z, 0.5f, 0.75f, lr_t, omd, EMA);
        elem(pp.w, gg.w, mm.w, vv.w, dd.w, ee.w, 0.5f, 0.75f, lr_t, omd, EMA);
        p[i] = pp; m[i] = mm; v[i] = vv;
        if (EMA) e[i] = ee;
    }
}

int main()
{
    const size_t n = 1695936;          // the flat count of TimitQCNN(10, 32) rounded up to a multiple of 4
    float *buf[6];
    std::vector<float> h(n);
    for (size_t i = 0; i < n; ++i) h[i] = 1e-3f * (float)((i * 2654435761u) % 2001) - 1.f;
    for (int b = 0; b < 6; ++b) { CK(hipMalloc(&buf[b], n * 4)); CK(hipMemcpy(buf[b], h.data(), n * 4, hipMemcpyHostToDevice)); }
    CK(hipMemset(buf[2], 0, n * 4)); CK(hipMemset(buf[3], 0, n * 4));
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    auto blocks = [](size_t k) { size_t x = (k + 255) / 256; return (unsigned)(x > 2048 ? 2048 : x); };
    for (int round = 0; round < 3; ++round)
        for (int form = 0; form < 4; ++form) {
            auto run = [&]() {
                switch (form) {
                case 0: hipLaunchKernelGGL(k4<false>, dim3(blocks(n)), dim3(256), 0, 0, buf[0], buf[1], buf[2], buf[3], buf[4], buf[5], n, 1e-4f, 1e-3f); break;
                case 1: hipLaunchKernelGGL(k16<false>, dim3(blocks(n / 4)), dim3(256), 0, 0, (float4 *)buf[0], (const float4 *)buf[1], (float4 *)buf[2], (float4 *)buf[3], (const float4 *)buf[4], (float4 *)buf[5], n / 4, 1e-4f, 1e-3f); break;
                case 2: hipLaunchKernelGGL(k4<true>, dim3(blocks(n)), dim3(256), 0, 0, buf[0], buf[1], buf[2], buf[3], buf[4], buf[5], n, 1e-4f, 1e-3f); break;
                case 3: hipLaunchKernelGGL(k16<true>, dim3(blocks(n / 4)), dim3(256), 0, 0, (float4 *)buf[0], (const float4 *)buf[1], (float4 *)buf[2], (float4 *)buf[3], (const float4 *)buf[4], (float4 *)buf[5], n / 4, 1e-4f, 1e-3f); break;
                }
            };
            for (int i = 0; i < 50; ++i) run();
            CK(hipDeviceSynchronize());
            CK(hipEventRecord(a, 0));
            for (int i = 0; i < 1000; ++i) run();
            CK(hipEventRecord(b, 0));
            CK(hipEventSynchronize(b));
            float ms = 0; CK(hipEventElapsedTime(&ms, a, b));
            static const char *names[] = {"4-byte", "16-byte", "4-byte+ema", "16-byte+ema"};
            printf("round %d %-12s %.2f us per launch\n", round, names[form], ms);
        }
    CK(hipGetLastError());
    return 0;
}
