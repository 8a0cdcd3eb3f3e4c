// row_transfer.hpp -- (rows, K) host images in the caller's element order <-> padded, optionally renumbered device planes:
// the transposing kernels and the staged copies around them (sw2d_device.hip, poisson2d_device.hip).
#pragma once
#include "device_buffer.hpp"

namespace bdg_dev {

// perm[k_caller] = device slot (NULL = identity). One thread per (row, element).
template <typename T>
__global__ void scatter_rows_kernel(const T* __restrict__ src, T* __restrict__ dst, int rows, int K, long long ld,
                                    const int* __restrict__ perm) {
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= static_cast<long long>(rows) * K) return;
    const long long r = t / K, k = t % K;
    dst[r * ld + (perm ? perm[k] : k)] = src[t];
}

template <typename T>
__global__ void gather_rows_kernel(const T* __restrict__ src, T* __restrict__ dst, int rows, int K, long long ld,
                                   const int* __restrict__ perm) {
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= static_cast<long long>(rows) * K) return;
    const long long r = t / K, k = t % K;
    dst[t] = src[r * ld + (perm ? perm[k] : k)];
}

// Where the rows go: K elements in planes of ld, through `perm` (device pointer, may be nullptr), on `stream`.
struct RowLayout {
    int K;
    long long ld;
    const int* perm;
    hipStream_t stream;
};

// host (rows, K) -> device rows at `dev`, staged through `staging` (rows * K entries of device memory)
template <typename T>
void uploadRows(const RowLayout& l, const T* host, T* dev, T* staging, int rows) {
    const size_t n = static_cast<size_t>(rows) * l.K;
    hipCheck(hipMemcpyAsync(staging, host, n * sizeof(T), hipMemcpyHostToDevice, l.stream), "H2D copy");
    hipLaunchKernelGGL((scatter_rows_kernel<T>), dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, l.stream, staging, dev,
                       rows, l.K, l.ld, l.perm);
    hipCheck(hipGetLastError(), "scatter_rows_kernel");
    hipCheck(hipStreamSynchronize(l.stream), "upload sync"); // the staging buffer is reused
}

template <typename T>
void downloadRows(const RowLayout& l, const T* dev, T* host, T* staging, int rows) {
    const size_t n = static_cast<size_t>(rows) * l.K;
    hipLaunchKernelGGL((gather_rows_kernel<T>), dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, l.stream, dev, staging,
                       rows, l.K, l.ld, l.perm);
    hipCheck(hipGetLastError(), "gather_rows_kernel");
    hipCheck(hipMemcpyAsync(host, staging, n * sizeof(T), hipMemcpyDeviceToHost, l.stream), "D2H copy");
    hipCheck(hipStreamSynchronize(l.stream), "download sync");
}

} // namespace bdg_dev
