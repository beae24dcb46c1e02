// replay_host.cpp -- the product's host entry points (kh_host_* of include/kimi_hip.h) replayed from a case file on exact-size
// heap buffers, for a build with AddressSanitizer and UBSan (tests/native_replay.py, tests/test_native_sanitized_host.py).
// Linked with csrc/common.hip, csrc/join.hip and csrc/section.hip.  It calls nothing that asks for a device and makes no HIP call.
#include "replay_io.h"

#include "../../include/kimi_hip.h"

static int64_t f_ccl26(const rp_call* c) {
  return kh_host_ccl26(A(0), (int)I(0), I(1), I(2), I(3), (uint32_t*)A(1));
}
static int64_t f_consolidate_paths(const rp_call* c) {
  return kh_host_consolidate_paths(I(0), (const int64_t*)A(0), (const int64_t*)A(1), (const uint32_t*)A(2), (const uint32_t*)A(3),
                                   (const float*)A(4), I(1), I(2), I(3), (float*)A(5), (float*)A(6), (uint32_t*)A(7), (int64_t*)A(8),
                                   (int64_t*)A(9));
}
static int64_t f_merge_components(const rp_call* c) {
  return kh_host_merge_components(I(0), (const int64_t*)A(0), (const int64_t*)A(1), (const int64_t*)A(2), (const float*)A(3),
                                  (const float*)A(4), (const uint32_t*)A(5), I(1), I(2), F(3), F(4), F(5), (float*)A(6), (float*)A(7),
                                  (uint32_t*)A(8));
}
static int64_t f_find_border_targets(const rp_call* c) {
  return kh_host_find_border_targets((const float*)A(0), (const uint32_t*)A(1), I(0), I(1), F(2), F(3), I(4), (float*)A(2),
                                     (int32_t*)A(3));
}
static int64_t f_resolve_holes(const rp_call* c) {
  return kh_host_resolve_holes(I(0), (const uint64_t*)A(0), (const uint32_t*)A(1), (const uint8_t*)A(2), I(1), (const uint64_t*)A(3),
                               (uint64_t*)A(4), (uint64_t*)A(5), (uint8_t*)A(6), (int64_t*)A(7));
}
static int64_t f_enclosed_regions(const rp_call* c) {
  return kh_host_enclosed_regions(I(0), (const uint64_t*)A(0), (const uint8_t*)A(1), I(1), (const uint64_t*)A(2), I(2),
                                  (const uint64_t*)A(3), (uint64_t*)A(4), (uint32_t*)A(5), I(3));
}
static int64_t f_join_plan(const rp_call* c) {
  return kh_host_join_plan(I(0), (const uint32_t*)A(0), (const uint64_t*)A(1), (const uint32_t*)A(2), (const float*)A(3), D(1),
                           (int)I(2), (uint32_t*)A(4));
}
static int64_t f_section_voxel(const rp_call* c) {
  return kh_host_section_voxel((const double*)A(0), (const double*)A(1), I(0), I(1), I(2), (double*)A(2), (double*)A(3),
                               (double*)A(4));
}

static const rp_entry TABLE[] = {
    {"kh_host_ccl26", f_ccl26},
    {"kh_host_consolidate_paths", f_consolidate_paths},
    {"kh_host_merge_components", f_merge_components},
    {"kh_host_find_border_targets", f_find_border_targets},
    {"kh_host_resolve_holes", f_resolve_holes},
    {"kh_host_enclosed_regions", f_enclosed_regions},
    {"kh_host_join_plan", f_join_plan},
    {"kh_host_section_voxel", f_section_voxel},
    {"selftest_overrun", rp_selftest_overrun},
};

int main(int argc, char** argv) { return rp_main(argc, argv, TABLE, sizeof TABLE / sizeof TABLE[0]); }
