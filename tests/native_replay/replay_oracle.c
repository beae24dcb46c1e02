/* replay_oracle.c -- the functions of oracle/kimi_oracle.c that oracle/__init__.py binds, replayed from a case file on exact-size
 * heap buffers, for a build with AddressSanitizer and UBSan (tests/native_replay.py, tests/test_native_sanitized_host.py).
 * Linked with oracle/kimi_oracle.c, which has no header: the prototypes below are its definitions'. */
#include "replay_io.h"

void ko_weights26(float wx, float wy, float wz, float* w);
int ko_edt(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz, int black_border,
           float* out);
int ko_edt_nd(const void* labels, int label_bytes, int ndim, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
              int black_border, float* out);
int ko_edf(const uint8_t* mask, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz, uint64_t source,
           float free_space_radius, float* out, uint64_t* max_loc, float* max_val);
void ko_set_voxel_graph(const uint32_t* g);
int ko_pdrf(const float* dbf, float* daf, int64_t n, float M, int exponent, float scale, float max_daf, float* out);
int64_t ko_target_order(const uint8_t* mask, const float* daf, int64_t n, uint32_t* order);
int ko_railroad(const float* f, int64_t sx, int64_t sy, int64_t sz, uint64_t target, float* d, uint64_t* path, int64_t* npath,
                int64_t* settled);
int ko_parental_field(const float* f, int64_t sx, int64_t sy, int64_t sz, uint64_t source, float* d, uint32_t* parents);
int ko_path_from_parents(const uint32_t* parents, int64_t n, uint64_t target, uint64_t* path, int64_t* npath);
int ko_field_distances(const float* f, int64_t sx, int64_t sy, int64_t sz, uint64_t source, float* d);
int ko_path_to_source(const float* f, const float* d, int64_t sx, int64_t sy, int64_t sz, uint64_t source, uint64_t target,
                      uint64_t* path, int64_t* npath);
int ko_invalidate_ball(uint8_t* field, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz, const uint64_t* sources,
                       const float* max_distances, int64_t nsrc, int64_t* invalidated, int64_t* heap_ops);
int ko_invalidate_ball_graph(uint8_t* field, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                             const uint64_t* sources, const float* max_distances, int64_t nsrc, const uint32_t* graph,
                             int64_t* invalidated, int64_t* heap_ops);
void ko_ball_radii(const float* dbf, const uint64_t* path, int64_t n, float scale, float constant, float* r);
int ko_invalidate_cube(uint8_t* labels, const float* dbf, int64_t sx, int64_t sy, int64_t sz, float wx, float wy, float wz,
                       const uint64_t* path, int64_t npath, float scale, float constant, int64_t* invalidated);
void ko_zero2inf(float* f, int64_t n);
void ko_inf2zero(float* f, int64_t n);
int64_t ko_first_label(const uint8_t* m, int64_t n);
int64_t ko_ccl26(const void* labels, int label_bytes, int64_t sx, int64_t sy, int64_t sz, uint32_t* out);

static int64_t f_weights26(const rp_call* c) { ko_weights26(F(0), F(1), F(2), (float*)A(0)); return 0; }
static int64_t f_edt(const rp_call* c) {
  return ko_edt(A(0), (int)I(0), I(1), I(2), I(3), F(4), F(5), F(6), (int)I(7), (float*)A(1));
}
static int64_t f_edt_nd(const rp_call* c) {
  return ko_edt_nd(A(0), (int)I(0), (int)I(1), I(2), I(3), I(4), F(5), F(6), F(7), (int)I(8), (float*)A(1));
}
static int64_t f_edf(const rp_call* c) {
  return ko_edf((const uint8_t*)A(0), I(0), I(1), I(2), F(3), F(4), F(5), (uint64_t)I(6), F(7), (float*)A(1), (uint64_t*)A(2),
                (float*)A(3));
}
static int64_t f_set_voxel_graph(const rp_call* c) { ko_set_voxel_graph((const uint32_t*)A(0)); return 0; }
static int64_t f_pdrf(const rp_call* c) {
  return ko_pdrf((const float*)A(0), (float*)A(1), I(0), F(1), (int)I(2), F(3), F(4), (float*)A(2));
}
static int64_t f_target_order(const rp_call* c) {
  return ko_target_order((const uint8_t*)A(0), (const float*)A(1), I(0), (uint32_t*)A(2));
}
static int64_t f_railroad(const rp_call* c) {
  return ko_railroad((const float*)A(0), I(0), I(1), I(2), (uint64_t)I(3), (float*)A(1), (uint64_t*)A(2), (int64_t*)A(3),
                     (int64_t*)A(4));
}
static int64_t f_parental_field(const rp_call* c) {
  return ko_parental_field((const float*)A(0), I(0), I(1), I(2), (uint64_t)I(3), (float*)A(1), (uint32_t*)A(2));
}
static int64_t f_path_from_parents(const rp_call* c) {
  return ko_path_from_parents((const uint32_t*)A(0), I(0), (uint64_t)I(1), (uint64_t*)A(1), (int64_t*)A(2));
}
static int64_t f_field_distances(const rp_call* c) {
  return ko_field_distances((const float*)A(0), I(0), I(1), I(2), (uint64_t)I(3), (float*)A(1));
}
static int64_t f_path_to_source(const rp_call* c) {
  return ko_path_to_source((const float*)A(0), (const float*)A(1), I(0), I(1), I(2), (uint64_t)I(3), (uint64_t)I(4), (uint64_t*)A(2),
                           (int64_t*)A(3));
}
static int64_t f_invalidate_ball(const rp_call* c) {
  return ko_invalidate_ball((uint8_t*)A(0), I(0), I(1), I(2), F(3), F(4), F(5), (const uint64_t*)A(1), (const float*)A(2), I(6),
                            (int64_t*)A(3), (int64_t*)A(4));
}
static int64_t f_invalidate_ball_graph(const rp_call* c) {
  return ko_invalidate_ball_graph((uint8_t*)A(0), I(0), I(1), I(2), F(3), F(4), F(5), (const uint64_t*)A(1), (const float*)A(2), I(6),
                                  (const uint32_t*)A(3), (int64_t*)A(4), (int64_t*)A(5));
}
static int64_t f_ball_radii(const rp_call* c) {
  ko_ball_radii((const float*)A(0), (const uint64_t*)A(1), I(0), F(1), F(2), (float*)A(2));
  return 0;
}
static int64_t f_invalidate_cube(const rp_call* c) {
  return ko_invalidate_cube((uint8_t*)A(0), (const float*)A(1), I(0), I(1), I(2), F(3), F(4), F(5), (const uint64_t*)A(2), I(6), F(7),
                            F(8), (int64_t*)A(3));
}
static int64_t f_zero2inf(const rp_call* c) { ko_zero2inf((float*)A(0), I(0)); return 0; }
static int64_t f_inf2zero(const rp_call* c) { ko_inf2zero((float*)A(0), I(0)); return 0; }
static int64_t f_first_label(const rp_call* c) { return ko_first_label((const uint8_t*)A(0), I(0)); }
static int64_t f_ccl26(const rp_call* c) { return ko_ccl26(A(0), (int)I(0), I(1), I(2), I(3), (uint32_t*)A(1)); }

static const rp_entry TABLE[] = {
    {"ko_weights26", f_weights26},
    {"ko_edt", f_edt},
    {"ko_edt_nd", f_edt_nd},
    {"ko_edf", f_edf},
    {"ko_set_voxel_graph", f_set_voxel_graph},
    {"ko_pdrf", f_pdrf},
    {"ko_target_order", f_target_order},
    {"ko_railroad", f_railroad},
    {"ko_parental_field", f_parental_field},
    {"ko_path_from_parents", f_path_from_parents},
    {"ko_field_distances", f_field_distances},
    {"ko_path_to_source", f_path_to_source},
    {"ko_invalidate_ball", f_invalidate_ball},
    {"ko_invalidate_ball_graph", f_invalidate_ball_graph},
    {"ko_ball_radii", f_ball_radii},
    {"ko_invalidate_cube", f_invalidate_cube},
    {"ko_zero2inf", f_zero2inf},
    {"ko_inf2zero", f_inf2zero},
    {"ko_first_label", f_first_label},
    {"ko_ccl26", f_ccl26},
    {"selftest_overrun", rp_selftest_overrun},
};

int main(int argc, char** argv) { return rp_main(argc, argv, TABLE, sizeof TABLE / sizeof TABLE[0]); }
