// Device plumbing shared by the HDP sources (sa_hdpgrid.hip, sa_hdpdist.hip): a device buffer that frees itself, and the
// device check every compute entry point starts with.
#ifndef SA_HDPDEV_H
#define SA_HDPDEV_H

#include <hip/hip_runtime.h>

#include "sa_scratch.h"

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void) hipFree(p); }
    int alloc(size_t bytes) { return hipMalloc(&p, bytes > 0 ? bytes : 8) == hipSuccess ? SA_OK : SA_ENOMEM; }
    int put(const void *src, size_t bytes) {
        if (alloc(bytes)) return SA_ENOMEM;
        return (bytes == 0 || hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) == hipSuccess) ? SA_OK : SA_ENODEVICE;
    }
};

// (the HDP calls answer a device that is out of range as they answer a missing one, the line on stderr included)
static inline int use_device(int device) {
    const int rc = sa_device_check(device);
    if (rc == SA_EINVAL) fprintf(stderr, SA_NO_DEVICE_LINE);
    if (rc) return SA_ENODEVICE;
    return hipSetDevice(device) == hipSuccess ? SA_OK : SA_ENODEVICE;
}

#endif
