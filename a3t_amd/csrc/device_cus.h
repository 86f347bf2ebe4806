// device_cus.h -- compute units of the current device: the grid size of the persistent kernels.
#pragma once
#include <hip/hip_runtime.h>

// Cached per device (a process may drive several GPUs); 256 without a device or when the query fails.
inline int device_cus() {
    static int n[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!n[dev]) {
        hipDeviceProp_t pr;
        if (hipGetDeviceProperties(&pr, dev) != hipSuccess) return 256;
        n[dev] = pr.multiProcessorCount > 0 ? pr.multiProcessorCount : 256;
    }
    return n[dev];
}
