// ward_value.h -- the fp32 value expressions of the reference's Ward clustering, shared by ward.hip (the large-N engine) and
// ward_many.hip (many small problems per launch).  Every translation unit that includes it must be compiled with
// -ffp-contract=off: each product, difference, sum and quotient below is rounded on its own, in the reference's order
// (clustering.go:37-40 MergeClusters, :136-157 WardDistance / DotFloat32).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#pragma clang fp contract(off)

// sum_k fl(fl(x_k - y_k)^2), strictly in k order, by ONE thread (d % 4 == 0, x and y 16-byte aligned): eight 16-byte loads of each row
// are in flight before the first of them is used -- the loads depend on nothing, but issued one k-group at a time each waits for the
// round trip of the previous one (a row pair took ~100 us that way)
__device__ __forceinline__ float ward_sqdist_thread(const float *__restrict__ x, const float *__restrict__ y, int d)
{
    const float4 *x4 = reinterpret_cast<const float4 *>(x), *y4 = reinterpret_cast<const float4 *>(y);
    const int ng = d >> 2;
    float s = 0.0f;
    int g = 0;
    for (; g + 8 <= ng; g += 8) {
        float4 xv[8], yv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            xv[q] = x4[g + q];
            yv[q] = y4[g + q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            float df = xv[q].x - yv[q].x; // clustering.go:139
            float p = df * df;            // :154 product (rounded)
            s = s + p;                    // :154 sum (rounded), strictly in k order
            df = xv[q].y - yv[q].y;
            p = df * df;
            s = s + p;
            df = xv[q].z - yv[q].z;
            p = df * df;
            s = s + p;
            df = xv[q].w - yv[q].w;
            p = df * df;
            s = s + p;
        }
    }
    for (; g < ng; ++g) {
        const float4 xv = x4[g], yv = y4[g];
        float df = xv.x - yv.x;
        float p = df * df;
        s = s + p;
        df = xv.y - yv.y;
        p = df * df;
        s = s + p;
        df = xv.z - yv.z;
        p = df * df;
        s = s + p;
        df = xv.w - yv.w;
        p = df * df;
        s = s + p;
    }
    return s;
}

// WardDistance of two clusters from their centroids (clustering.go:136-157): what the exact update kernels compute per entry
__device__ __forceinline__ float ward_pair_value(const float *__restrict__ x, const float *__restrict__ y, int d, int sx, int sy)
{
    float s = 0.0f;
    if ((d & 3) == 0) {
        s = ward_sqdist_thread(x, y, d);
    } else {
        for (int k = 0; k < d; ++k) {
            const float df = x[k] - y[k];
            const float p = df * df;
            s = s + p;
        }
    }
    const float num = (float)((int64_t)sx * (int64_t)sy); // :142
    const float den = (float)(sx + sy);                    // :143
    return (num / den) * s;                                // :144
}

// WardDistance's scaling of a finished sum (clustering.go:142-144)
__device__ __forceinline__ float ward_scale(float s, int sx, int sy)
{
    const float num = (float)((int64_t)sx * (int64_t)sy); // :142
    const float den = (float)(sx + sy);                    // :143
    return (num / den) * s;                                // :144
}

// MergeClusters' centroid element (clustering.go:37-40): (float(sa) * Ca[k] + float(sb) * Cb[k]) / float(sa + sb), each operation rounded
__device__ __forceinline__ float ward_merge_elem(float fa, float ca, float fb, float cb, float fs)
{
    const float pa = fa * ca;
    const float pb = fb * cb;
    const float sm = pa + pb;
    return sm / fs;
}
