// A recording stand-in for the HIP runtime: the host objects of libmgacbam (csrc/api_*.hip) link against it with clang++ instead of
// libamdhip64, so every entry point runs on a machine without a GPU and each launch it would make is printed instead -- kernel
// (mangled name, from the registration the objects do at start-up), grid, block, dynamic LDS, stream.  tools/launch_plan.py builds it.
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <map>
#include <string>

static std::map<const void*, std::string>& names() { static std::map<const void*, std::string> m; return m; }
static int g_occupancy = 4;   // workgroups per CU the occupancy query answers (0: k_gate is never eligible)
static int g_fail_next = 0;

extern "C" {
void stub_set_occupancy(int per_cu) { g_occupancy = per_cu; }
void stub_fail_next_launch(void) { g_fail_next = 1; }

void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_stub, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
  names()[host_stub] = device_name;
}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
hipError_t __hipPushCallConfiguration(dim3, dim3, size_t, hipStream_t) { return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3*, dim3*, size_t*, hipStream_t*) { return hipSuccess; }

hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void**, size_t lds, hipStream_t st) {
  auto it = names().find(f);
  printf("  launch %s grid=%u,%u,%u block=%u,%u,%u lds=%zu stream=%p%s\n", it == names().end() ? "?" : it->second.c_str(), grid.x, grid.y,
         grid.z, block.x, block.y, block.z, lds, static_cast<void*>(st), g_fail_next ? " -> fails" : "");
  if (g_fail_next) { g_fail_next = 0; return hipErrorLaunchFailure; }
  return hipSuccess;
}
hipError_t hipGetDevice(int* dev) { *dev = 0; return hipSuccess; }
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t a, int) { *v = a == hipDeviceAttributeMultiprocessorCount ? 256 : 0; return hipSuccess; }
hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int* n, const void*, int, size_t) { *n = g_occupancy; return hipSuccess; }
hipError_t hipFuncSetAttribute(const void* f, hipFuncAttribute, int value) {
  auto it = names().find(f);
  printf("  attribute %s max-dynamic-lds=%d\n", it == names().end() ? "?" : it->second.c_str(), value);
  return hipSuccess;
}
const char* hipGetErrorString(hipError_t e) { return e == hipErrorLaunchFailure ? "launch failure (stand-in)" : "error (stand-in)"; }
}
