// avr_kpaths_slot.h — where each k_paths instantiation of avr_kpaths_list.h sits in the
// context's kernel table, which one a render selects, and what it is called. Plain C++ (no
// HIP): the C-ABI unit fills and indexes the table through it, and tests/test_kpaths_slot.py
// checks the table on the host.
#pragma once

namespace avr {
namespace kp {

// Template arguments as the list spells them: medium 0 GridMedium, 1 Homogeneous / Cloud,
// 3 NanoVDB, 4 RGBGridMedium; sampler 0 IndependentSampler, 2 / 3 ZSobolSampler with a 32-bit /
// 64-bit sample index. Their dense indices in the table:
constexpr int medium_index(int medium_arg) { return medium_arg == 3 ? 1 : (medium_arg == 4 ? 2 : (medium_arg == 1 ? 3 : 0)); }
constexpr int sampler_index(int sampler_arg) { return sampler_arg == 0 ? 0 : (sampler_arg == 2 ? 1 : 2); }

constexpr int kNumSlots = 2 * 2 * 4 * 3 * 2 * 2;   // 192; RGBGridMedium's 24 gray slots alias its non-gray entries

constexpr int slot(bool fast, bool image, int medium_idx, int sampler_idx, bool emissive, bool gray) {
    return ((((int(fast) * 2 + int(image)) * 4 + medium_idx) * 3 + sampler_idx) * 2 + int(emissive)) * 2 + int(gray);
}
// X(emissive, gray, sampler, medium, image, fast) of AVR_KP_ALL -> its slot and its name, the
// instantiation as a profiler prints it (avr_last_kernel)
constexpr int slot_of(bool emissive, bool gray, int sampler_arg, int medium_arg, bool image, bool fast) {
    return slot(fast, image, medium_index(medium_arg), sampler_index(sampler_arg), emissive, gray);
}
#define AVR_KP_NAME(em, gr, zs, med, im, fa) "k_paths<" #em ", " #gr ", " #zs ", " #med ", " #im ", " #fa ">"

// RGBGridMedium carries per-voxel spectra and has no gray instantiation: after the list is
// expanded into a table, its gray slots take the 4-wavelength entries beside them
template <typename T>
void alias_rgb_gray(T *table) {
    for (int k = 0; k < kNumSlots; k += 2)
        if ((k / 12) % 4 == medium_index(4)) table[k + 1] = table[k];
}

// The context's medium type (0 grid, 1 homogeneous, 2 cloud, 3 NanoVDB, 4 RGB grid) and sampler
// (kind 0 independent, 1 ZSobol; wide: the 64-bit index) as template arguments
constexpr int medium_arg(int medium_type) { return medium_type == 3 ? 3 : (medium_type == 4 ? 4 : (medium_type == 1 || medium_type == 2 ? 1 : 0)); }
constexpr int sampler_arg(int sampler_kind, bool wide) { return sampler_kind == 0 ? 0 : (wide ? 3 : 2); }
// The parked instantiations (template arguments as the list spells them): gray GridMedium without
// emission or image light. They read the density through the fat layout alone, fixed at compile
// time (k_paths' collision block).
constexpr bool parked(bool emissive, bool gray, int medium_arg, bool image) {
    return gray && medium_arg == 0 && !emissive && !image;
}
// The slot a render launches. image: image lights or the power light sampler (the kImage
// instantiation also carries the latter's pick); gray: sigma_a and sigma_s constant over all
// wavelengths; fat: a GridMedium's density has its fat copy (the default layout). A medium that
// would run a parked instantiation but has the linear or the bricked layout runs the general
// instantiation beside it instead (kImage: every light kind, every layout at run time).
constexpr int select(bool fast, bool image, int medium_type, int sampler_kind, bool wide, bool emissive, bool gray,
                     bool fat = true) {
    return slot(fast, image || (!fat && parked(emissive, gray, medium_arg(medium_type), image)),
                medium_index(medium_arg(medium_type)), sampler_index(sampler_arg(sampler_kind, wide)), emissive, gray);
}

}  // namespace kp
}  // namespace avr
