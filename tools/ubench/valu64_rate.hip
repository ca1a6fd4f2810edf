// development microbenchmark: what the 64-bit address arithmetic of a per-lane table read costs to issue, per CU and by waves per SIMD:
// v_mad_u64_u32, v_lshl_add_u64, v_lshlrev_b64 and the 32-bit forms that replace them (v_mul_lo_u32, v_mad_u32_u24, v_lshl_add_u32,
// v_lshlrev_b32), against v_fma_f32 as the reference row; and a global_load_dwordx4 in both address forms ({64-bit vector address, off}
// and {32-bit vector offset, scalar base}) on a 1 KiB block that stays in the vector cache (the address path, not the memory, is the question)
// build: hipcc -O3 --offload-arch=gfx950 tools/ubench/valu64_rate.hip -o valu64_rate ; run it on an MI355X
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

enum { FMA, MAD64, LSHLADD64, LSHL64, MULLO, MAD24, LSHLADD32, LSHL32, LOAD_VADDR, LOAD_SADDR, N_MODES };
static const char* const NAMES[N_MODES] = {"v_fma_f32", "v_mad_u64_u32", "v_lshl_add_u64", "v_lshlrev_b64", "v_mul_lo_u32", "v_mad_u32_u24",
                                           "v_lshl_add_u32", "v_lshlrev_b32", "global_load_dwordx4 v[a:a+1], off", "global_load_dwordx4 vOff, s[b:b+1]"};

template <int MODE>
__global__ void __launch_bounds__(256) k(unsigned* out, const f4* __restrict__ tab, int iters) {
    const unsigned lane = threadIdx.x & 63u;
    float f0 = (float)threadIdx.x, f1 = 1.f, f2 = 2.f, f3 = 3.f, fm = 1.0000001f;
    u64 a0 = threadIdx.x, a1 = 1, a2 = 2, a3 = 3, ab = blockIdx.x;
    unsigned u0 = threadIdx.x, u1 = 1, u2 = 2, u3 = 3, um = 3u + blockIdx.x;
    const unsigned off = lane * 16u;                               // the wave's 64 lanes read one 1 KiB block
    const u64 vaddr = (u64)tab + off;
    f4 r0 = {0, 0, 0, 0}, r1 = r0, r2 = r0, r3 = r0;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (MODE == FMA)
                asm volatile("v_fma_f32 %0, %0, %4, %4\n v_fma_f32 %1, %1, %4, %4\n v_fma_f32 %2, %2, %4, %4\n v_fma_f32 %3, %3, %4, %4" : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3) : "v"(fm));
            else if (MODE == MAD64)
                asm volatile("v_mad_u64_u32 %0, vcc, %4, %5, %0\n v_mad_u64_u32 %1, vcc, %4, %5, %1\n v_mad_u64_u32 %2, vcc, %4, %5, %2\n v_mad_u64_u32 %3, vcc, %4, %5, %3"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(u0), "v"(um) : "vcc");
            else if (MODE == LSHLADD64)
                asm volatile("v_lshl_add_u64 %0, %0, 1, %4\n v_lshl_add_u64 %1, %1, 1, %4\n v_lshl_add_u64 %2, %2, 1, %4\n v_lshl_add_u64 %3, %3, 1, %4" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(ab));
            else if (MODE == LSHL64)
                asm volatile("v_lshlrev_b64 %0, 1, %0\n v_lshlrev_b64 %1, 1, %1\n v_lshlrev_b64 %2, 1, %2\n v_lshlrev_b64 %3, 1, %3" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));
            else if (MODE == MULLO)
                asm volatile("v_mul_lo_u32 %0, %0, %4\n v_mul_lo_u32 %1, %1, %4\n v_mul_lo_u32 %2, %2, %4\n v_mul_lo_u32 %3, %3, %4" : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3) : "v"(um));
            else if (MODE == MAD24)
                asm volatile("v_mad_u32_u24 %0, %0, %4, %4\n v_mad_u32_u24 %1, %1, %4, %4\n v_mad_u32_u24 %2, %2, %4, %4\n v_mad_u32_u24 %3, %3, %4, %4" : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3) : "v"(um));
            else if (MODE == LSHLADD32)
                asm volatile("v_lshl_add_u32 %0, %0, 1, %4\n v_lshl_add_u32 %1, %1, 1, %4\n v_lshl_add_u32 %2, %2, 1, %4\n v_lshl_add_u32 %3, %3, 1, %4" : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3) : "v"(um));
            else if (MODE == LSHL32)
                asm volatile("v_lshlrev_b32 %0, 1, %0\n v_lshlrev_b32 %1, 1, %1\n v_lshlrev_b32 %2, 1, %2\n v_lshlrev_b32 %3, 1, %3" : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3));
            else if (MODE == LOAD_VADDR)
                asm volatile("global_load_dwordx4 %0, %4, off\n global_load_dwordx4 %1, %4, off\n global_load_dwordx4 %2, %4, off\n global_load_dwordx4 %3, %4, off"
                             : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3) : "v"(vaddr) : "memory");
            else
                asm volatile("global_load_dwordx4 %0, %4, %5\n global_load_dwordx4 %1, %4, %5\n global_load_dwordx4 %2, %4, %5\n global_load_dwordx4 %3, %4, %5"
                             : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3) : "v"(off), "s"(tab) : "memory");
        }
        if (MODE >= LOAD_VADDR) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (f0 + f1 + f2 + f3 == 12345.f || a0 + a1 + a2 + a3 == 0x123456789ull || u0 + u1 + u2 + u3 == 0x87654321u || r0.x + r1.y + r2.z + r3.w == 12345.f) out[0] = 1;
}

template <int MODE>
static void row(unsigned* d, const f4* tab, int iters) {
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    for (int wps = 1; wps <= 8; wps *= 2) {                     // waves per SIMD: wps blocks of 256 threads per CU
        const int grid = 256 * wps;
        float best = 1e30f;
        for (int rep = 0; rep < 3; ++rep) {
            hipEventRecord(a);
            k<MODE><<<grid, 256>>>(d, tab, iters);
            hipEventRecord(b); hipEventSynchronize(b);
            if (hipGetLastError() != hipSuccess) { printf("launch failed\n"); exit(1); }
            float ms; hipEventElapsedTime(&ms, a, b); if (ms < best) best = ms;
        }
        const double inst = 64.0 * iters * wps * 4;             // per CU
        printf("%-36s waves/SIMD %d  %.3f ms  %.3f instr/ns/CU  (at 2.4 GHz: %.3f per cycle per CU, %.2f cycles per instruction per SIMD)\n", NAMES[MODE], wps, best,
               inst / (best * 1e6), inst / (best * 1e6) / 2.4, 4.0 * 2.4 * best * 1e6 / inst);
    }
}

int main() {
    setvbuf(stdout, nullptr, _IONBF, 0);
    unsigned* d; hipMalloc(&d, 4);
    f4* tab; hipMalloc(&tab, 4096); hipMemset(tab, 0, 4096);     // lanes read bytes 0 .. 1023
    const int iters = 1000;
    row<FMA>(d, tab, iters); row<MAD64>(d, tab, iters); row<LSHLADD64>(d, tab, iters); row<LSHL64>(d, tab, iters);
    row<MULLO>(d, tab, iters); row<MAD24>(d, tab, iters); row<LSHLADD32>(d, tab, iters); row<LSHL32>(d, tab, iters);
    row<LOAD_VADDR>(d, tab, iters); row<LOAD_SADDR>(d, tab, iters);
    hipDeviceSynchronize();
    return 0;
}
