// Device plumbing shared by the HDP sources (sa_hdpgrid.hip, sa_hdpdist.hip): a device buffer that frees itself, and the
// device check every compute entry point starts with.
#ifndef SA_HDPDEV_H
#define SA_HDPDEV_H

#include <hip/hip_runtime.h>

#include <cstdio>

#include "signalalign_hip.h"

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void) hipFree(p); }
    int alloc(size_t bytes) { return hipMalloc(&p, bytes > 0 ? bytes : 8) == hipSuccess ? SA_OK : SA_ENOMEM; }
    int put(const void *src, size_t bytes) {
        if (alloc(bytes)) return SA_ENOMEM;
        return (bytes == 0 || hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) == hipSuccess) ? SA_OK : SA_ENODEVICE;
    }
};

static inline int use_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        (void) hipGetLastError();
        fprintf(stderr, "[signalalign_hip] no HIP device available; this library has no CPU fallback\n");
        return SA_ENODEVICE;
    }
    return hipSetDevice(device) == hipSuccess ? SA_OK : SA_ENODEVICE;
}

#endif
