// The split-f16 tile families: one row per id range.  Everything that turns a tile id into a family, a mode, a name, a kernel
// or a launch goes through family_of; the rules about which launch may run which tile are Plan::tile_legal's (plan_tiles.cpp).
#include "rtod_internal.h"

namespace rtod {

static const TileFamily kFamilies[TF_COUNT] = {
    {TF_GENERIC, 0, HV_COUNT, 0, 0, conv_f16s3_variant_info, conv_f16s3_kernel_name, launch_conv_f16s3},
    // band modes >= BAND_LDS_MODES are the bandd tiles: the only ones of that family with an f16 or a raw-sum instance.  launch_conv_band_f16s3 hands them to
    // launch_conv_bandd_f16s3(mode - BAND_LDS_MODES) before anything else, also the wide tile of the non-band layers
    {TF_BAND, BAND_VARIANT_BASE, BAND_MODES, BAND_LDS_MODES, BAND_LDS_MODES, conv_band_mode_info, conv_band_kernel_name, launch_conv_band_f16s3},
    {TF_RING, RING_VARIANT_BASE, RING_MODES, RING_MODES, RING_MODES, conv_ring_mode_info, conv_ring_kernel_name, launch_conv_ring_f16s3},
    {TF_PWD, PWD_VARIANT_BASE, PWD_MODES, 0, 0, conv_pwd_mode_info, conv_pwd_kernel_name, launch_conv_pwd_f16s3},
    {TF_PATCH, PATCH_VARIANT_BASE, PATCH_MODES, PATCH_MODES, PATCH_MODES, conv_patch_mode_info, conv_patch_kernel_name, launch_conv_patch_f16s3},
    {TF_C16, C16_VARIANT_BASE, C16_MODES, 0, 0, conv_c16_mode_info, conv_c16_kernel_name, launch_conv_c16_f16s3},
    {TF_KS, KS_VARIANT_BASE, KS_MODES, 0, KS_MODES, conv_ks_mode_info, conv_ks_kernel_name, launch_conv_ks_f16s3},
};
static_assert(HV_COUNT <= BAND_VARIANT_BASE, "generic tile ids end where the band family's begin");
static_assert(BAND_VARIANT_BASE + BAND_MODES <= RING_VARIANT_BASE, "band tile ids end where the ring family's begin");
static_assert(RING_VARIANT_BASE + RING_MODES <= PWD_VARIANT_BASE, "ring tile ids end where the pwd family's begin");
static_assert(PWD_VARIANT_BASE + PWD_MODES <= PATCH_VARIANT_BASE, "pwd tile ids end where the patch family's begin");
static_assert(PATCH_VARIANT_BASE + PATCH_MODES <= STEM2_VARIANT && STEM2_VARIANT < C16_VARIANT_BASE, "the fused stem's reported id lies between the patch and narrow families");
static_assert(C16_VARIANT_BASE + C16_MODES <= KS_VARIANT_BASE, "narrow tile ids end where the K-sliced family's begin");

TileRef family_of(int v) {
    for (const TileFamily& f : kFamilies)
        if (v >= f.base && v < f.base + f.modes) return {&f, v - f.base};
    return {nullptr, 0};
}

const TileFamily& tile_family(int family) { return kFamilies[family]; }

}  // namespace rtod
