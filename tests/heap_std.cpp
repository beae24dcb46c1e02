// heap_std.cpp -- a script of kh_heap_script's records (include/kimi_hip.h) run on the std::priority_queue of the libstdc++ that is
// installed: the witness tests/heap_ref.py is pinned to (tests/test_heap_ref_host.py).  No capacity: the caller removes the pushes
// a capacity would refuse.  usage: heap_std script.bin pops.bin dumps.bin   (dumps without mirror words)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <queue>
#include <vector>

struct Node { float dist; uint32_t payload, source; };
struct Cmp { bool operator()(const Node& a, const Node& b) const { return a.dist >= b.dist; } };
struct Queue : std::priority_queue<Node, std::vector<Node>, Cmp> {
  const std::vector<Node>& container() const { return c; }
};
static float as_float(uint32_t bits) { float f; std::memcpy(&f, &bits, 4); return f; }
static uint32_t as_bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  std::vector<uint32_t> ops;
  if (FILE* f = std::fopen(argv[1], "rb")) {
    uint32_t rec[4];
    while (std::fread(rec, 4, 4, f) == 4) ops.insert(ops.end(), rec, rec + 4);
    std::fclose(f);
  } else return 2;
  std::vector<uint32_t> pops, dumps;
  Queue q;
  const size_t nops = ops.size() / 4;
  for (size_t i = 0; i < nops; i++) {
    const uint32_t op = ops[4 * i], a = ops[4 * i + 1], b = ops[4 * i + 2], c = ops[4 * i + 3];
    if (op == 0) q.push(Node{as_float(a), b, c});
    else if (op == 1) {
      if (q.empty()) return 3;
      const Node t = q.top();
      const uint32_t rec[4] = {as_bits(t.dist), t.payload, t.source, (uint32_t)q.size()};
      pops.insert(pops.end(), rec, rec + 4);
      q.pop();
    } else if (op == 2) {
      dumps.push_back((uint32_t)q.size());
      dumps.push_back((uint32_t)i);
      if (!(a & 1u))
        for (const Node& n : q.container()) {
          const uint32_t rec[4] = {as_bits(n.dist), n.payload, n.source, 0u};
          dumps.insert(dumps.end(), rec, rec + 4);
        }
    } else return 3;
  }
  FILE* fp = std::fopen(argv[2], "wb");
  FILE* fd = std::fopen(argv[3], "wb");
  if (!fp || !fd) return 2;
  std::fwrite(pops.data(), 4, pops.size(), fp);
  std::fwrite(dumps.data(), 4, dumps.size(), fd);
  return (std::fclose(fp) | std::fclose(fd)) ? 2 : 0;
}
