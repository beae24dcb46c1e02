/* replay_io.h -- the case file and the result file of the two replay programs (replay_host.cpp, replay_oracle.c): plain C, no
 * dependencies.  tests/native_replay.py writes the one and reads the other.
 *
 * A program is run as `prog CASE RESULT`, or as `prog --list` to print the function names it knows, one per line.
 *
 * Case file, little endian, no padding:
 *   u32 magic 0x3150524B ("KRP1")
 *   u32 narrays;  per array: u64 element size, u64 count, then count * size raw bytes
 *   u32 ncalls;   per call:  u32 length of the name, the name;
 *                            u32 nscalars, per scalar: u8 'i' (an int64 follows) or 'd' (a float64 follows);
 *                            u32 nargs,    per array argument: i32 index into the arrays, -1 = pass NULL
 * Every array lives in a malloc of its own of exactly count * size bytes (malloc(0) for an empty one) that the bytes are read
 * straight into, so that under AddressSanitizer the first byte behind the contract's size is poisoned.  An output array comes with
 * the writer's canary pattern as its bytes.  The calls are made in order on the one set of arrays (more than one call: the
 * oracle's ko_set_voxel_graph around a search).
 *
 * Result file: u32 ncalls, per call the i64 return value (0 for a void function);
 *              u32 narrays, per array u64 bytes and the WHOLE buffer as it is after the calls.                               */
#ifndef REPLAY_IO_H
#define REPLAY_IO_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define RP_MAX_ARGS 24
#define RP_MAGIC 0x3150524Bu

typedef struct rp_array {
  uint64_t size, count;
  void* p;
} rp_array;

typedef struct rp_call {
  char name[64];
  uint32_t nscalars, nargs;
  char kind[RP_MAX_ARGS];
  int64_t i[RP_MAX_ARGS];
  double d[RP_MAX_ARGS];
  rp_array* arg[RP_MAX_ARGS];   /* NULL: pass NULL */
} rp_call;

typedef int64_t (*rp_fn)(const rp_call*);
typedef struct rp_entry {
  const char* name;
  rp_fn fn;
} rp_entry;

static void rp_die(const char* what) {
  fprintf(stderr, "replay: %s\n", what);
  exit(2);
}

static void rp_read(FILE* f, void* to, size_t n) {
  if (n && fread(to, 1, n, f) != n) rp_die("case file too short");
}

static int64_t rp_i(const rp_call* c, uint32_t k) {
  if (k >= c->nscalars || c->kind[k] != 'i') rp_die("scalar is not an integer of the case");
  return c->i[k];
}
static double rp_d(const rp_call* c, uint32_t k) {
  if (k >= c->nscalars || c->kind[k] != 'd') rp_die("scalar is not a float of the case");
  return c->d[k];
}
static void* rp_a(const rp_call* c, uint32_t k) {
  if (k >= c->nargs) rp_die("array argument missing from the case");
  return c->arg[k] ? c->arg[k]->p : NULL;
}

/* the check that the harness can fail: one element behind the end of array argument 0 */
static int64_t rp_selftest_overrun(const rp_call* c) {
  if (c->nargs < 1 || !c->arg[0]) rp_die("selftest_overrun wants an array");
  volatile unsigned char* p = (volatile unsigned char*)c->arg[0]->p;
  const uint64_t end = c->arg[0]->size * c->arg[0]->count;
  for (uint64_t b = 0; b < c->arg[0]->size; b++) p[end + b] = 0x5A;
  return 0;
}

static int rp_main(int argc, char** argv, const rp_entry* table, size_t nentries) {
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    for (size_t e = 0; e < nentries; e++) puts(table[e].name);
    return 0;
  }
  if (argc != 3) rp_die("usage: prog CASE RESULT | prog --list");
  FILE* f = fopen(argv[1], "rb");
  if (!f) rp_die("cannot open the case file");
  uint32_t magic = 0, narrays = 0, ncalls = 0;
  rp_read(f, &magic, 4);
  if (magic != RP_MAGIC) rp_die("not a case file");
  rp_read(f, &narrays, 4);
  rp_array* arrays = (rp_array*)malloc(sizeof(rp_array) * (narrays ? narrays : 1));
  if (!arrays) rp_die("out of memory");
  for (uint32_t a = 0; a < narrays; a++) {
    rp_read(f, &arrays[a].size, 8);
    rp_read(f, &arrays[a].count, 8);
    const size_t bytes = (size_t)(arrays[a].size * arrays[a].count);
    arrays[a].p = malloc(bytes);              /* exactly the contract's bytes; malloc(0) is a poisoned non-null pointer under ASan */
    if (!arrays[a].p) rp_die("out of memory");
    rp_read(f, arrays[a].p, bytes);
  }
  rp_read(f, &ncalls, 4);
  int64_t* rets = (int64_t*)malloc(sizeof(int64_t) * (ncalls ? ncalls : 1));
  if (!rets) rp_die("out of memory");
  for (uint32_t k = 0; k < ncalls; k++) {
    rp_call c;
    memset(&c, 0, sizeof c);
    uint32_t len = 0;
    rp_read(f, &len, 4);
    if (len >= sizeof c.name) rp_die("name too long");
    rp_read(f, c.name, len);
    rp_read(f, &c.nscalars, 4);
    if (c.nscalars > RP_MAX_ARGS) rp_die("too many scalars");
    for (uint32_t s = 0; s < c.nscalars; s++) {
      rp_read(f, &c.kind[s], 1);
      if (c.kind[s] == 'i') rp_read(f, &c.i[s], 8);
      else if (c.kind[s] == 'd') rp_read(f, &c.d[s], 8);
      else rp_die("unknown scalar kind");
    }
    rp_read(f, &c.nargs, 4);
    if (c.nargs > RP_MAX_ARGS) rp_die("too many arrays");
    for (uint32_t s = 0; s < c.nargs; s++) {
      int32_t at = 0;
      rp_read(f, &at, 4);
      if (at >= (int32_t)narrays) rp_die("array index outside the case");
      c.arg[s] = at < 0 ? NULL : &arrays[at];
    }
    rp_fn fn = NULL;
    for (size_t e = 0; e < nentries; e++)
      if (!strcmp(table[e].name, c.name)) fn = table[e].fn;
    if (!fn) rp_die("unknown function");
    rets[k] = fn(&c);
  }
  fclose(f);
  FILE* o = fopen(argv[2], "wb");
  if (!o) rp_die("cannot open the result file");
  fwrite(&ncalls, 4, 1, o);
  fwrite(rets, 8, ncalls, o);
  fwrite(&narrays, 4, 1, o);
  for (uint32_t a = 0; a < narrays; a++) {
    const uint64_t bytes = arrays[a].size * arrays[a].count;
    fwrite(&bytes, 8, 1, o);
    if (bytes) fwrite(arrays[a].p, 1, (size_t)bytes, o);
  }
  if (fclose(o) != 0) rp_die("cannot write the result file");
  for (uint32_t a = 0; a < narrays; a++) free(arrays[a].p);
  free(arrays);
  free(rets);
  return 0;
}

#define I(k) rp_i(c, k)
#define D(k) rp_d(c, k)
#define F(k) ((float)rp_d(c, k))
#define A(k) rp_a(c, k)

#endif
