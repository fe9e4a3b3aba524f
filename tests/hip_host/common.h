// Host stand-in for csrc/common.h (tests/test_augment_host_cpu.py): compiles a kernel source with g++ and runs it with
// one OS thread per work-item and a pthread barrier for __syncthreads, so that AddressSanitizer / UBSan see every LDS and
// buffer access of the kernel's index arithmetic.  Only what csrc/crop_coeff.h and csrc/crop_augment.hip use.
#pragma once
#include <pthread.h>
#include <stdint.h>

#include <thread>
#include <vector>
#define MMMOT_OK 0
#define MMMOT_EINVAL (-1)
struct int4 { int x, y, z, w; };
struct float4 { float x, y, z, w; };
static inline float4 make_float4(float a, float b, float c, float d) { return float4{a, b, c, d}; }
struct dim3 {
  unsigned x, y, z;
  dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
static thread_local dim3 threadIdx;
static thread_local dim3 blockIdx;
static pthread_barrier_t g_barrier;
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define __syncthreads() pthread_barrier_wait(&g_barrier)
static inline double __ddiv_rn(double a, double b) { return a / b; }  // compile with -ffp-contract=off
static inline double __dmul_rn(double a, double b) { return a * b; }
static inline double __dadd_rn(double a, double b) { return a + b; }
static inline double __dsub_rn(double a, double b) { return a - b; }
static inline float __fdiv_rn(float a, float b) { return a / b; }
static inline float __fsub_rn(float a, float b) { return a - b; }
typedef int hipError_t;
#define hipSuccess 0
typedef void* hipStream_t;
static inline int hipGetLastError() { return 0; }
static inline int mm_check(hipError_t e) { return e; }
template <class F>
static void host_launch(dim3 grid, dim3 block, F fn) {
  // block.x threads, made once per launch; together they walk the workgroups one after the other (the __shared__
  // arrays are statics: one workgroup at a time), a barrier between two workgroups
  pthread_barrier_init(&g_barrier, nullptr, block.x);
  std::vector<std::thread> th;
  for (unsigned i = 0; i < block.x; ++i)
    th.emplace_back([=] {
      threadIdx = dim3(i, 0, 0);
      for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
          blockIdx = dim3(bx, by, 0);
          fn();
          pthread_barrier_wait(&g_barrier);
        }
    });
  for (auto& t : th) t.join();
  pthread_barrier_destroy(&g_barrier);
}
#define hipLaunchKernelGGL(k, grid, block, shmem, stream, ...) host_launch(grid, block, [=] { k(__VA_ARGS__); })
