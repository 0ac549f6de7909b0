// fp_sep.h -- a product, a sum or a difference that is rounded on its own, whatever the expression around it.
//
// Several contracts of this library (include/sr355.h: sr_resize's float taps, sr_back_projection, sr_edge_guided, sr_noise_sigma, sr_adam,
// the patch gathers' v * mul + add, ...) promise the bits of a NumPy or OpenCV evaluation that rounds every product and every sum separately.
// hipcc compiles device code with -ffp-contract=fast: wherever a product feeds a sum it may emit one fused multiply-add, which rounds once.
// The __fmul_rn / __fadd_rn / __dmul_rn / __dadd_rn intrinsics do NOT prevent that: their header bodies are plain `*` and `+`, they inline,
// and the backend fuses the two instructions like any others -- the intrinsic spelling of a * b + c compiles to v_fmac_f32.  A
// `#pragma clang fp contract(off)` at the call site does not help either: it governs the operators written in its own scope, not those of
// an inlined callee.
//
// The helpers below therefore carry the pragma in their own bodies: the instruction each one emits has no `contract` flag, and the backend
// fuses a product into a sum only when both carry it.  Use them wherever a contract names two roundings; write fmaf() / fma() /
// __fmaf_rn() where one rounding is meant; leave plain operators where the contract is a tolerance.  Division and square root are never
// contracted: __fdiv_rn / __ddiv_rn / sqrtf stay as they are.  tests/test_rounding_contracts_cpu.py lists every kernel that uses either
// spelling, and tests/test_rounding_contracts_gpu.py holds them to the bits on inputs where an fma would differ.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float mul_sep(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_sep(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float sub_sep(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ double mul_sep(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double add_sep(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ double sub_sep(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}
