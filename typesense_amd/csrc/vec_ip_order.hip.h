// vec_ip_order.hip.h — the exact inner-product distance of one (query, row) pair in hnswlib's own summation order, as device functions.
// Included by vec_kernels.hip.h (k-NN re-score, by-id distances, HNSW traversal) and by kw_vq_sort.hip.h (the `_vector_query` sort slot of the
// keyword kernels): one definition, so every path returns the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tsgpu {

// hnswlib InnerProductSpace::get_dist_func arithmetic for one (query, row) pair, evaluated by a 16-lane group
// (space_ip.h: InnerProductSIMD16Ext / SIMD4Ext / *Residuals): products and sums rounded separately (no FMA),
// 16 (or 4) running lane sums, sequential horizontal add. sub = lane index inside the group (0..15); every lane of
// the group returns the distance. qs = the query (LDS or global), x = the row in global memory.
// Contraction is switched off lexically in every function below (the __fmul_rn/__fadd_rn header intrinsics are plain
// operators compiled under the default -ffp-contract=fast and DO fuse after inlining).
__device__ inline float ip_mul_add(float acc, float a, float b) {
#pragma clang fp contract(off)
    const float pr = a * b;
    return acc + pr;
}
__device__ inline float ip_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ inline float ip_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
// ---- hnswlib InnerProductSpace summation orders (space_ip.h; restated in oracle/oracle_index.h: ip_simd16ext / ip_simd4ext) ----
// `lanes` = the SIMD width hnswlib was COMPILED for, which fixes the order the products are added in: 4 = SSE (the reference's stock
// flags pass no -march: CMakeLists.txt:8, BUILD:81-88 — element i accumulates in lane i % 4, final T0+T1+T2+T3; library default),
// 8 = AVX (lane i % 8, T0+..+T7; dims % 4: __m256 over the 16-multiples folded lo+hi into an __m128 for the rest), 16 = AVX-512
// (lane i % 16, T0+..+T15; dims % 4 as AVX). Option "vec_ip_lanes". Every form multiplies and adds with separate roundings.
//
// Generic form: 16 GPU lanes per row (sub = lane & 15), any dim; lanes sub < L own the L accumulator lanes (a strided scalar walk:
// the by-id / odd-dimension paths, not the batched re-score).
__device__ inline float ip_acc_strided(float acc, const float* qs, const float* __restrict__ x, uint32_t from, uint32_t to, uint32_t sub, uint32_t L) {
    if (sub < L) for (uint32_t i = from + sub; i < to; i += L) acc = ip_mul_add(acc, qs[i], x[i]);
    return acc;
}
__device__ inline float ip_hsum(float accl, uint32_t L) {                 // T0 + T1 + .. + T(L-1), left to right, over the 16-lane group's first L lanes
    const int b0 = (int)(threadIdx.x & 48u);
    float sum = 0.0f;
    if (L == 4) {
        const float l0 = __shfl(accl, b0), l1 = __shfl(accl, b0 + 1), l2 = __shfl(accl, b0 + 2), l3 = __shfl(accl, b0 + 3);
        return ip_add(ip_add(ip_add(l0, l1), l2), l3);                    // (SSE form: no leading 0 + ..)
    }
#pragma unroll
    for (int l = 0; l < 16; l++) { const float v = __shfl(accl, b0 + l); if ((uint32_t)l < L) sum = ip_add(sum, v); }
    return sum;
}
__device__ inline float ip_simd16ext(const float* qs, const float* __restrict__ x, uint32_t qty, uint32_t sub, uint32_t L) {    // qty % 16 == 0
    return ip_hsum(ip_acc_strided(0.0f, qs, x, 0, qty, sub, L), L);
}
__device__ inline float ip_simd4ext(const float* qs, const float* __restrict__ x, uint32_t qty, uint32_t sub, uint32_t L) {     // qty % 4 == 0
    if (L == 4) return ip_hsum(ip_acc_strided(0.0f, qs, x, 0, qty, sub, 4), 4);
    const uint32_t q16 = qty / 16 * 16;                                   // InnerProductSIMD4ExtAVX
    const float a8 = ip_acc_strided(0.0f, qs, x, 0, q16, sub, 8);
    const float hi = __shfl(a8, (int)((threadIdx.x & 48u) + ((sub + 4) & 15)));
    const float s4 = ip_add(a8, hi);                                      // lanes 0..3: lo + hi
    return ip_hsum(ip_acc_strided(s4, qs, x, q16, qty, sub, 4), 4);
}
__device__ inline float ip_scalar(const float* qs, const float* __restrict__ x, uint32_t off, uint32_t n) {
    float r = 0.0f;
    for (uint32_t i = 0; i < n; i++) r = ip_mul_add(r, qs[off + i], x[off + i]);
    return r;
}
__device__ inline float ip_distance_group16(const float* qs, const float* __restrict__ x, uint32_t dim, uint32_t sub, uint32_t L) {
    if (dim % 16 == 0) return ip_add(1.0f, -ip_simd16ext(qs, x, dim, sub, L));
    if (dim % 4 == 0) return ip_add(1.0f, -ip_simd4ext(qs, x, dim, sub, L));
    if (dim > 16) { const uint32_t qn = dim >> 4 << 4; const float a1 = ip_simd16ext(qs, x, qn, sub, L); return ip_add(1.0f, -ip_add(a1, ip_scalar(qs, x, qn, dim - qn))); }
    if (dim > 4) { const uint32_t qn = dim >> 2 << 2; const float a1 = ip_simd4ext(qs, x, qn, sub, L); return ip_add(1.0f, -ip_add(a1, ip_scalar(qs, x, qn, dim - qn))); }
    return ip_add(1.0f, -ip_scalar(qs, x, 0, dim));
}

// Fast form for dim % 16 == 0 (the batched re-score and the graph traversal): FOUR GPU lanes per row, 16-byte loads; lane v of the
// quad loads elements 16 j + 4 v .. + 3 of every 16-element block j and forms their four products p[v][0..3]; a wavefront covers 16
// rows per round. Who ADDS which product follows the order:
//   L = 16: element 16 j + 4 v + c belongs to accumulator lane 4 v + c -> lane v keeps four chains of its own products;
//   L = 8:  accumulator lane (4 v + c) % 8 -> quad lanes 0 / 1 own lanes 0..3 / 4..7 and add their own products, then those of lane
//           v + 2 (one quad_perm exchange per block);
//   L = 4:  accumulator lane c takes p[0][c], p[1][c], p[2][c], p[3][c] in that order -> the 4 x 4 block of products is TRANSPOSED
//           inside the quad (two butterfly stages over quad_perm), quad lane c owns accumulator lane c.
// Same products, same order inside every accumulator lane, same left-to-right final sum as the CPU forms; U = blocks requested per
// lane before the first product is consumed (memory-level parallelism: a 768-dimension row costs two round trips).
__device__ inline float quad_xor1(float v) { return __uint_as_float((uint32_t)__builtin_amdgcn_mov_dpp((int)__float_as_uint(v), 0xB1, 0xF, 0xF, true)); }   // quad_perm [1,0,3,2]
__device__ inline float quad_xor2(float v) { return __uint_as_float((uint32_t)__builtin_amdgcn_mov_dpp((int)__float_as_uint(v), 0x4E, 0xF, 0xF, true)); }   // quad_perm [2,3,0,1]
template <int U>
__device__ inline float ip_dot16_quad(const float* qs, const float* __restrict__ x, uint32_t n16, uint32_t v, uint32_t L) {
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const bool odd = (v & 1) != 0, hi = (v & 2) != 0;
    for (uint32_t i = 0; i < n16; i += 16 * U) {
        float4 xv[U];
#pragma unroll
        for (int u = 0; u < U; u++) xv[u] = *(const float4*)(x + (i + 16 * u < n16 ? i + 16 * u : 0) + 4 * v);
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (i + 16 * u < n16) {                                       // (uniform per block: n16, i, u are wave-uniform)
                const float4 qv = *(const float4*)(qs + i + 16 * u + 4 * v);
                if (L == 16) {
                    acc[0] = ip_mul_add(acc[0], qv.x, xv[u].x); acc[1] = ip_mul_add(acc[1], qv.y, xv[u].y);
                    acc[2] = ip_mul_add(acc[2], qv.z, xv[u].z); acc[3] = ip_mul_add(acc[3], qv.w, xv[u].w);
                } else {
                    float p[4] = {ip_mul(qv.x, xv[u].x), ip_mul(qv.y, xv[u].y), ip_mul(qv.z, xv[u].z), ip_mul(qv.w, xv[u].w)};
                    if (L == 8) {
#pragma unroll
                        for (int c = 0; c < 4; c++) acc[c] = ip_add(ip_add(acc[c], p[c]), quad_xor2(p[c]));      // (meaningful on quad lanes 0 and 1)
                    } else {
#pragma unroll
                        for (int k = 0; k < 2; k++) {                     // stage A: swap bit 0 of (lane, component)
                            const float recv = quad_xor1(odd ? p[2 * k] : p[2 * k + 1]);
                            if (odd) p[2 * k] = recv; else p[2 * k + 1] = recv;
                        }
#pragma unroll
                        for (int k = 0; k < 2; k++) {                     // stage B: swap bit 1
                            const float recv = quad_xor2(hi ? p[k] : p[k + 2]);
                            if (hi) p[k] = recv; else p[k + 2] = recv;
                        }
                        acc[0] = ip_add(ip_add(ip_add(ip_add(acc[0], p[0]), p[1]), p[2]), p[3]);                  // quad lane c = accumulator lane c
                    }
                }
            }
        }
    }
    const int q0 = (int)(threadIdx.x & 60u);
    if (L == 4) {
        const float t0 = __shfl(acc[0], q0), t1 = __shfl(acc[0], q0 + 1), t2 = __shfl(acc[0], q0 + 2), t3 = __shfl(acc[0], q0 + 3);
        return ip_add(ip_add(ip_add(t0, t1), t2), t3);
    }
    float sum = 0.0f;
    const int nl = L == 16 ? 4 : 2;                                       // quad lanes holding accumulator lanes, four each
#pragma unroll
    for (int vv = 0; vv < 4; vv++)
#pragma unroll
        for (int c = 0; c < 4; c++) { const float t = __shfl(acc[c], q0 + vv); if (vv < nl) sum = ip_add(sum, t); }
    return sum;
}

}  // namespace tsgpu
