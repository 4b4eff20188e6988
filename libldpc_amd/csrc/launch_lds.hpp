// launch_lds.hpp — the launch of a kernel that takes dynamic LDS (host side; .hip files only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ldpc_amd
{

// Raises the kernel's dynamic-LDS limit to lds_bytes (without it a launch stops at 64 KB of the CU's 160), enqueues the
// kernel on `stream` (hipStream_t passed as void*) and returns the hipError_t as int.
template <typename... Params, typename... Args>
int launch_with_lds(void (*kernel)(Params...), dim3 grid, dim3 block, uint32_t lds_bytes, void *stream, const Args &...args)
{
    const hipError_t e =
        hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds_bytes));
    if (e != hipSuccess)
    {
        (void)hipGetLastError(); // (reported here: the next launch's check must not find it again)
        return e;
    }
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, static_cast<hipStream_t>(stream), args...);
    return hipGetLastError();
}

} // namespace ldpc_amd
