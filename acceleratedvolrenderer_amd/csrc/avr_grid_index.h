// Index arithmetic of the GridMedium density layouts: pbrt's linear SampledGrid, the fat
// footprint copy and the 8^3 apron bricks (DevMedium in avr_kernels.hip). Shared by the device
// kernels and the host; standalone so the host tests compile it with g++ and run the very
// expressions the kernels run (tests/test_grid_index.py).
#pragma once

#include <cstddef>
#include <cstdint>

#ifndef AVR_HD
#define AVR_HD __host__ __device__ __forceinline__
#endif

namespace avr {

// 24 x 24 -> low 32 bits multiply: only the low 24 bits of each operand count. One
// v_mul_u32_u24 on the device (a quarter-rate v_mul_lo_u32 otherwise); the host evaluates the
// same truncation, so a caller whose operands do not fit fails on the host as on the device.
AVR_HD uint32_t mul_u24(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return (uint32_t)((a & 0xffffffu) * (b & 0xffffffu));
#endif
}

// Linear index of voxel (x, y, z), 0 <= x < nx ..., in pbrt's x-fastest SampledGrid order.
// 32-bit arithmetic for grids of at most 2^31 voxels (the condition is made of kernel
// arguments: wave-uniform), 64-bit beyond.
AVR_HD size_t grid_linear_index(int nx, int ny, int nz, int x, int y, int z) {
    if ((uint64_t)nx * (uint64_t)ny * (uint64_t)nz <= (1ull << 31))
        return (size_t)(((uint32_t)z * (uint32_t)ny + (uint32_t)y) * (uint32_t)nx + (uint32_t)x);
    return ((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx + (size_t)x;
}

// True when fat_entry_index() may take the 24-bit multiplies: every operand fits 24 bits, i.e.
// iz + 1 and ny + 1 (both below the next bound), their sum term (iz + 1)(ny + 1) + iy + 1 <
// (ny + 1)(nz + 1) < 2^24 and nx + 1 < 2^24; and the whole index fits 31 bits (the float4 index
// is twice it). Cubes to 1289^3 qualify; a grid thin in x and wide in y and z (1 x 4096 x 4096)
// does not, however few entries it has.
AVR_HD bool fat_index_is_24bit(int nx, int ny, int nz) {
    const uint64_t ex = (uint64_t)nx + 1, ey = (uint64_t)ny + 1, ez = (uint64_t)nz + 1;
    return ey * ez < (1ull << 24) && ex < (1ull << 24) && ex * ey * ez < (1ull << 31);
}

// Entry index of footprint (ix, iy, iz), -1 <= ix < nx ..., in the fat copy of a grid
// (nx, ny, nz): entries in x-fastest order over (nx + 1, ny + 1, nz + 1); an entry is two
// float4. The branch condition is made of kernel arguments only (scalar, wave-uniform).
AVR_HD size_t fat_entry_index(int nx, int ny, int nz, int ix, int iy, int iz) {
    const uint32_t ex = (uint32_t)nx + 1, ey = (uint32_t)ny + 1;
    if (fat_index_is_24bit(nx, ny, nz))
        return (size_t)(mul_u24(mul_u24((uint32_t)(iz + 1), ey) + (uint32_t)(iy + 1), ex) + (uint32_t)(ix + 1));
    return ((size_t)(iz + 1) * ey + (size_t)(iy + 1)) * ex + (size_t)(ix + 1);
}

// Bricked copy: 9^3 = 729 apron values per brick, padded to 23 x 128-B lines
constexpr int kBrickFloats = 736;

// Float offset of the base tap of footprint u = (ix + 1, iy + 1, iz + 1), 0 <= ux <= nx ..., in
// the bricked copy: brick u >> 3 of (nb[0], nb[1], nb[2]) bricks in x-fastest order, then the
// apron-local u & 7 in the brick's 9^3 values (x fastest). The other seven taps lie 1, 9, 10,
// 81, 82, 90 and 91 floats further on.
AVR_HD size_t brick_float_offset(const int nb[3], int ux, int uy, int uz) {
    const size_t b = ((size_t)(uz >> 3) * (size_t)nb[1] + (size_t)(uy >> 3)) * (size_t)nb[0] + (size_t)(ux >> 3);
    return b * (size_t)kBrickFloats + (size_t)(((uz & 7) * 9 + (uy & 7)) * 9 + (ux & 7));
}

}  // namespace avr
