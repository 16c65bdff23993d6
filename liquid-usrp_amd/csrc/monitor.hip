// monitor.hip -- channel monitor for gfx950: per-channel level, peak and averaged periodogram of the channelizer's output.
//
// One more consumer of the (channel, tile) granules the synchronizers read: chan[tile][channel][MCRX_TILE] cf32, 128 bytes = one
// cache line per granule, so a wave that owns one channel reads whole lines and never a neighbour's.  Per launch and channel the
// logical stream is  carry (the samples of the segment the previous launch left unfinished, whole granules) ++ the new tiles;  it is cut
// into segments of nfft samples and shared out over `nsplit` waves per channel.  Per segment: window, nfft-point transform, |X|^2 in
// fp32; the sum over segments per bin and the sum of |x|^2 over the new samples in fp64, one accumulator per lane.  Every wave
// leaves its partial sums in HBM; monitor_fold_kernel adds them in split order to the handle's running sums -- no atomics on
// floating-point data, the same pushes give the same bits.
//
//   monitor64_kernel       nfft = 64: a segment is four granules, one sample per lane; the transform is the 64-point radix-2 DIF across
//                          the wave of lean_prims.hpp (six exchange stages, no LDS memory, no barrier); lane l ends with bin bitrev6(l)
//   monitor_generic_kernel nfft = 16, 32, 128, 256: a wave per workgroup, the windowed segment in LDS, every lane sums its bins directly
//                          (nfft complex multiply-adds per bin).  Correctness path, not tuned.
#include "devmath.h"
#include "kernels.h"

namespace mcrx {
#include "lean_prims.hpp"

#define MON_WV 64
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

// |x|^2, written out so that every site rounds alike (one product, one fused multiply-add): level and peak do not depend on where a push is cut
__device__ __forceinline__ float mon_pow(float re, float im) { return fmaf(re, re, im * im); }
// logical sample i of channel c: the carry first, then the new tiles
__device__ __forceinline__ float2 mon_sample(const MonArgs &a, uint32_t c, uint32_t i)
{
    if (i < a.carry_len) return a.carry_in[(size_t)c * a.carry_cap + i];
    const uint32_t j = i - a.carry_len;
    return a.chan[((size_t)(a.t0 + (j >> MCRX_TILE_SH)) * a.stride + a.off + c) * MCRX_TILE_S + (j & (MCRX_TILE_S - 1))];
}
// w[n] of the window (0 rectangular, 1 Hann, 2 Hamming)
__device__ __forceinline__ float mon_window(uint32_t window, uint32_t n, uint32_t nfft)
{
    if (window == 0) return 1.f;
    const float c = cospif(2.0f * (float)n / (float)nfft);
    return window == 1 ? 0.5f - 0.5f * c : 0.54f - 0.46f * c;
}
__device__ __forceinline__ double mon_wave_sum(double v)
{
#pragma unroll
    for (int h = 1; h < MON_WV; h <<= 1) v += __shfl_xor(v, h, MON_WV);
    return v;
}
__device__ __forceinline__ float mon_wave_max(float v)
{
#pragma unroll
    for (int h = 1; h < MON_WV; h <<= 1) v = fmaxf(v, __shfl_xor(v, h, MON_WV));
    return v;
}
// what the last wave of a channel does besides its segments: the samples behind the last whole segment are counted (where new) and
// become the next launch's carry
__device__ __forceinline__ void mon_tail(const MonArgs &a, uint32_t c, uint32_t l, uint32_t done, uint32_t total, double &lev, float &pk)
{
    for (uint32_t i = done + l; i < total; i += MON_WV) {
        const float2 x = mon_sample(a, c, i);
        if (i >= a.carry_len) { const float p = mon_pow(x.x, x.y); lev += (double)p; pk = fmaxf(pk, p); }
        a.carry_out[(size_t)c * a.carry_cap + (i - done)] = x;
    }
}

__global__ __launch_bounds__(256) void monitor64_kernel(MonArgs a)
{
    using namespace lean;
    const uint32_t l = (uint32_t)lane_id();
    const uint32_t w = blockIdx.x * (blockDim.x / MON_WV) + (threadIdx.x / MON_WV);        // wave-uniform: (channel, split)
    if (w >= a.nch * a.nsplit) return;
    const uint32_t c = w / a.nsplit, k = w % a.nsplit;
    const uint32_t total = a.carry_len + a.ntiles * MCRX_TILE_S, S = total / 64u;
    const uint32_t s0 = (uint32_t)((uint64_t)S * k / a.nsplit), s1 = (uint32_t)((uint64_t)S * (k + 1) / a.nsplit);
    const int bp32 = (int)((l ^ 32u) << 2);
    v2f tw[6], sgp[3];                       // stage twiddles (1 in the lower lanes); butterfly signs, two stages to a pair
#pragma unroll
    for (int st = 0; st < 6; st++) {
        const uint32_t h = 32u >> st;
        const bool up = (l & h) != 0;
        float sn, cs;
        sincospif((float)(l & (h - 1)) / (float)h, &sn, &cs);
        tw[st].x = up ? cs : 1.f; tw[st].y = up ? -sn : 0.f;
        if (st & 1) sgp[st >> 1].y = up ? -1.f : 1.f; else sgp[st >> 1].x = up ? -1.f : 1.f;
    }
    const float wl = mon_window(a.window, l, 64u);
    double acc = 0.0, lev = 0.0;
    float pk = 0.f;
    auto segment = [&](float2 x, bool fresh) {
        const float p = mon_pow(x.x, x.y);
        if (fresh) { lev += (double)p; pk = fmaxf(pk, p); }
        v2f y; y.x = x.x * wl; y.y = x.y * wl;
        y = fft64<63>(y, tw, sgp, bp32);
        acc += (double)mon_pow(y.x, y.y);
    };
    uint32_t s = s0;
    if (s == 0 && s1 > 0 && a.carry_len) { segment(mon_sample(a, c, l), l >= a.carry_len); s = 1; }      // the segment the carry begins
    // every other segment lies in the new tiles: lane l's sample of segment s is element l & 15 of granule 4 s + l / 16 (- the carry's)
    const float2 *base = a.chan + ((size_t)a.t0 * a.stride + a.off + c) * MCRX_TILE_S + (l & (MCRX_TILE_S - 1));
    const size_t tile_step = (size_t)a.stride * MCRX_TILE_S;
    const uint32_t g0 = (l >> MCRX_TILE_SH), gc = a.carry_len >> MCRX_TILE_SH;
    for (; s + 4 <= s1; s += 4) {            // four segments' loads in flight
        float2 x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) x[u] = base[(size_t)(4u * (s + u) + g0 - gc) * tile_step];
#pragma unroll
        for (int u = 0; u < 4; u++) segment(x[u], true);
    }
    for (; s < s1; s++) segment(base[(size_t)(4u * s + g0 - gc) * tile_step], true);
    if (k == a.nsplit - 1) mon_tail(a, c, l, S * 64u, total, lev, pk);
    a.part_psd[((size_t)k * a.nch + c) * 64u + (uint32_t)lane_k<64>((int)l)] = acc;
    lev = mon_wave_sum(lev); pk = mon_wave_max(pk);
    if (l == 0) { a.part_level[(size_t)k * a.nch + c] = lev; a.part_peak[(size_t)k * a.nch + c] = pk; }
}

__global__ __launch_bounds__(MON_WV) void monitor_generic_kernel(MonArgs a)
{
    __shared__ float2 seg[256], twd[256];
    const uint32_t l = threadIdx.x, nfft = a.nfft, mask = nfft - 1;
    const uint32_t c = blockIdx.x / a.nsplit, k = blockIdx.x % a.nsplit;
    const uint32_t total = a.carry_len + a.ntiles * MCRX_TILE_S, S = total / nfft;
    const uint32_t s0 = (uint32_t)((uint64_t)S * k / a.nsplit), s1 = (uint32_t)((uint64_t)S * (k + 1) / a.nsplit);
    float wl[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t n = l + MON_WV * r;
        wl[r] = mon_window(a.window, n & mask, nfft);
        if (n < nfft) { float sn, cs; sincospif(2.0f * (float)n / (float)nfft, &sn, &cs); twd[n] = make_float2(cs, -sn); }
    }
    double acc[4] = { 0.0, 0.0, 0.0, 0.0 }, lev = 0.0;
    float pk = 0.f;
    __syncthreads();
    for (uint32_t s = s0; s < s1; s++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint32_t n = l + MON_WV * r;
            if (n < nfft) {
                const uint32_t i = s * nfft + n;
                const float2 x = mon_sample(a, c, i);
                if (i >= a.carry_len) { const float p = mon_pow(x.x, x.y); lev += (double)p; pk = fmaxf(pk, p); }
                seg[n] = make_float2(x.x * wl[r], x.y * wl[r]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint32_t bin = l + MON_WV * r;
            if (bin < nfft) {
                float re[4] = { 0.f, 0.f, 0.f, 0.f }, im[4] = { 0.f, 0.f, 0.f, 0.f };      // four interleaved sums: shorter chains of roundings
                for (uint32_t n = 0; n < nfft; n += 4) {
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const float2 x = seg[n + u], t = twd[(bin * (n + u)) & mask];
                        re[u] = fmaf(x.x, t.x, fmaf(-x.y, t.y, re[u]));
                        im[u] = fmaf(x.x, t.y, fmaf(x.y, t.x, im[u]));
                    }
                }
                const float xr = (re[0] + re[1]) + (re[2] + re[3]), xi = (im[0] + im[1]) + (im[2] + im[3]);
                acc[r] += (double)mon_pow(xr, xi);
            }
        }
        __syncthreads();
    }
    if (k == a.nsplit - 1) mon_tail(a, c, l, S * nfft, total, lev, pk);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t bin = l + MON_WV * r;
        if (bin < nfft) a.part_psd[((size_t)k * a.nch + c) * nfft + bin] = acc[r];
    }
    lev = mon_wave_sum(lev); pk = mon_wave_max(pk);
    if (l == 0) { a.part_level[(size_t)k * a.nch + c] = lev; a.part_peak[(size_t)k * a.nch + c] = pk; }
}

// the splits' partial sums into the running sums, in split order
__global__ __launch_bounds__(256) void monitor_fold_kernel(MonArgs a)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nb = (size_t)a.nch * a.nfft;
    if (i < nb) {
        double s = 0.0;
        for (uint32_t k = 0; k < a.nsplit; k++) s += a.part_psd[(size_t)k * nb + i];
        a.psd[i] += s;
    } else if (i < nb + a.nch) {
        const size_t c = i - nb;
        double s = 0.0; float p = a.peak[c];
        for (uint32_t k = 0; k < a.nsplit; k++) { s += a.part_level[(size_t)k * a.nch + c]; p = fmaxf(p, a.part_peak[(size_t)k * a.nch + c]); }
        a.level[c] += s; a.peak[c] = p;
    }
}

hipError_t monitor_launch(const MonArgs &a, hipStream_t st)
{
    if (a.nch == 0 || a.nsplit == 0) return hipErrorInvalidValue;
    if (a.nfft == 64) {
        const uint32_t waves = a.nch * a.nsplit;
        hipLaunchKernelGGL(monitor64_kernel, dim3((waves + 3) / 4), dim3(256), 0, st, a);
    } else {
        if (a.nfft != 16 && a.nfft != 32 && a.nfft != 128 && a.nfft != 256) return hipErrorInvalidValue;
        hipLaunchKernelGGL(monitor_generic_kernel, dim3(a.nch * a.nsplit), dim3(MON_WV), 0, st, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t n = (size_t)a.nch * a.nfft + a.nch;
    hipLaunchKernelGGL(monitor_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace mcrx
