// Host stand-ins for the few HIP declarations patchmatchnet_amd/csrc/plan.hip uses, so that the plan recorder compiles and runs as
// plain C++ under AddressSanitizer / UBSan (tests/plan_host/plan_host_test.cpp, built and run by tests/test_plan_host.py).
// hipLaunchKernel does not launch: it logs (kernel, stream, first argument's bytes) for the test to read.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/pmn_hip.h"

struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
typedef void* hipStream_t;
enum hipError_t { hipSuccess = 0, hipErrorUnknown = 999 };

struct StubLaunch {
    const void* func;
    void* stream;
    long long arg0;  // the first argument read as a long long (the test passes one)
    unsigned grid_x;
};
static std::vector<StubLaunch> stub_launches;
static bool stub_fail_launch = false;

static inline hipError_t hipGetDevice(int* dev) {
    *dev = 0;
    return hipSuccess;
}
static inline hipError_t hipGetLastError() { return hipSuccess; }
static inline const char* hipKernelNameRefByPtr(const void*, hipStream_t) { return "stub_kernel"; }
static inline hipError_t hipLaunchKernel(const void* func, dim3 grid, dim3, void** args, size_t, hipStream_t stream) {
    if (stub_fail_launch) return hipErrorUnknown;
    stub_launches.push_back(StubLaunch{func, stream, *static_cast<long long*>(args[0]), grid.x});
    return hipSuccess;
}
