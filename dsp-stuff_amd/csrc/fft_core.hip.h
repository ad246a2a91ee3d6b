// fft_core.hip.h -- the banks' shared device code for complex arithmetic and the in-place FFT of a RUN of channels
// (spectrum_kernels.hip, convolve_kernels.hip; pitch_kernels.hip takes cmul / cadd / csub only).  Device only, hipcc only.
//
// A workgroup of ST threads transforms Q adjacent channels at once.  The Q transforms of m = 2^LOGM complex points live in ONE
// LDS buffer A[point][q] (q fastest, as in memory) and are done in place: a pass reads all its points into registers, the
// workgroup meets, then it writes them in Stockham order, so the output is in natural order with no second buffer and the run
// is twice as wide as two buffers would allow.  Radix-4 passes and one radix-2 pass when log2 m is odd; twiddles from a table
// of 2m points rounded once from f64 (bank_common.hip.h twiddles(); none in the first pass, where they are all 1).
#pragma once

#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// one in-place Stockham pass of radix R over the Q transforms of m = 2^LOGM points in A[point][q], by ST threads; NS = the
// product of the radices before it; tw is the table of 2m points, so exp(-2 pi i t / m) = tw[2t]
template <int LOGM, int Q, int ST, int R, int NS>
__device__ __forceinline__ void fft_pass(float2 *A, const float2 *__restrict__ tw) {
    constexpr int n = 1 << LOGM, NR = n / R, IT = NR * Q / ST;
    static_assert(NR * Q % ST == 0, "every thread does the same number of butterflies");
    float2 v[IT][R];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int b = threadIdx.x + i * ST, q = b % Q, j = b / Q;
#pragma unroll
        for (int r = 0; r < R; ++r) v[i][r] = A[(j + r * NR) * Q + q];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int b = threadIdx.x + i * ST, q = b % Q, j = b / Q;
        const int k = j & (NS - 1);
        float2 *u = v[i];
        if (NS > 1) {
#pragma unroll
            for (int r = 1; r < R; ++r) u[r] = cmul(u[r], tw[2 * (k * r * (n / (NS * R)))]);
        }
        if (R == 2) {
            const float2 a = u[0];
            u[0] = cadd(a, u[1]);
            u[1] = csub(a, u[1]);
        } else {
            const float2 a0 = cadd(u[0], u[2]), a1 = csub(u[0], u[2]), a2 = cadd(u[1], u[3]), a3 = csub(u[1], u[3]);
            const float2 ja3 = make_float2(a3.y, -a3.x);                                   // -i * a3
            u[0] = cadd(a0, a2);
            u[1] = cadd(a1, ja3);
            u[2] = csub(a0, a2);
            u[3] = csub(a1, ja3);
        }
        const int d = (j - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) A[(d + r * NS) * Q + q] = u[r];
    }
    __syncthreads();
}

// the passes from NS on: fft_all<LOGM, Q, ST, 1> is the whole transform (LOGM = 7: radix 4, 4, 4, 2)
template <int LOGM, int Q, int ST, int NS>
__device__ __forceinline__ void fft_all(float2 *A, const float2 *__restrict__ tw) {
    constexpr int m = 1 << LOGM;
    if constexpr (NS * 4 <= m) {
        fft_pass<LOGM, Q, ST, 4, NS>(A, tw);
        fft_all<LOGM, Q, ST, NS * 4>(A, tw);
    } else if constexpr (NS * 2 <= m) {
        fft_pass<LOGM, Q, ST, 2, NS>(A, tw);
    }
}

}  // namespace
