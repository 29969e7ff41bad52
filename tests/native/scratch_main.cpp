// The scratch layout of csrc/scratch.h on the host, compiled by g++ with AddressSanitizer + UndefinedBehaviorSanitizer.
//     scratch_main
// Layouts of mixed element types -- bytes, int32, doubles, a 40-byte struct of doubles, a 32-byte struct of int32, a 12-byte
// struct of int32 (whose end is no multiple of a double's alignment) -- with the counts 0, 1, 3, 15, 16, 17 in several orders.
// Per layout: the rule of the header (order, disjointness, alignment, bytes(), empty spans, runs), then a malloc of exactly
// bytes() in which every element of every region is written through Span::in and, after all writes, read back: an overflow is
// ASan's failure, a misaligned access UBSan's.  One case is pgo_loop_support's work buffer at E = n_sel = nc = 1.
// Built and run by tests/test_scratch_native.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pgo.h"
#include "scratch.h"

namespace {
struct D5 {
  double v[5];
};
struct I8 {
  int32_t v[8];
};
struct I3 {
  int32_t v[3];
};
static_assert(sizeof(D5) == 40 && sizeof(I8) == 32 && sizeof(I3) == 12, "the sizes the test is about");

long n_checks = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    ++n_checks;                                                      \
    if (!(cond)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

// element k of region r holds value(r, k) in every scalar of it
int value(int r, int64_t k) { return (int)((r * 37 + k * 5 + 1) % 120); }
void set(uint8_t& x, int v) { x = (uint8_t)v; }
void set(int32_t& x, int v) { x = v; }
void set(double& x, int v) { x = v; }
void set(pgo_loop_support_stats& x, int v) { x.n_pairs_total = v, x.n_selected = v, x.n_supported = v, x.max_pairs = v, x._pad = v; }
void set(pgo_loop_support_record& x, int v) { x.selected = v, x.n_pairs = v, x.n_consistent = v, x.best = v, x.q_min = v; }
template <class T>
void set(T& x, int v) {
  for (auto& s : x.v) set(s, v);
}
bool is(const uint8_t& x, int v) { return x == (uint8_t)v; }
bool is(const int32_t& x, int v) { return x == v; }
bool is(const double& x, int v) { return x == v; }
bool is(const pgo_loop_support_stats& x, int v) { return x.n_pairs_total == v && x.n_selected == v && x.n_supported == v && x.max_pairs == v && x._pad == v; }
bool is(const pgo_loop_support_record& x, int v) { return x.selected == v && x.n_pairs == v && x.n_consistent == v && x.best == v && x.q_min == v; }
template <class T>
bool is(const T& x, int v) {
  bool ok = true;
  for (const auto& s : x.v) ok = ok && is(s, v);
  return ok;
}

struct Region {   // a span without its type
  int64_t offset, count, bytes, end, align;
  void (*write)(void* base, int64_t offset, int64_t count, int r);
  bool (*read)(const void* base, int64_t offset, int64_t count, int r);
};

template <class T>
Region add(pgo::Layout* L, int64_t count) {
  const int64_t before = L->bytes();
  const pgo::Span<T> s = L->add<T>(count);
  CHECK(s.count == count && s.bytes() == count * (int64_t)sizeof(T) && s.end() == s.offset + s.bytes());
  CHECK(count > 0 || L->bytes() == before);   // an empty span takes no room
  Region R;
  R.offset = s.offset;
  R.count = count;
  R.bytes = s.bytes();
  R.end = s.end();
  R.align = alignof(T) > 16 ? (int64_t)alignof(T) : 16;
  R.write = [](void* base, int64_t offset, int64_t n, int r) {
    T* p = pgo::Span<T>{offset, n}.in(base);
    for (int64_t k = 0; k < n; ++k) set(p[k], value(r, k));
  };
  R.read = [](const void* base, int64_t offset, int64_t n, int r) {
    const T* p = pgo::Span<T>{offset, n}.in(base);
    bool ok = true;
    for (int64_t k = 0; k < n; ++k) ok = ok && is(p[k], value(r, k));
    return ok;
  };
  return R;
}

constexpr int N_TYPES = 6;
Region add_type(pgo::Layout* L, int type, int64_t count) {
  switch (type) {
    case 0: return add<uint8_t>(L, count);
    case 1: return add<int32_t>(L, count);
    case 2: return add<double>(L, count);
    case 3: return add<D5>(L, count);
    case 4: return add<I8>(L, count);
    default: return add<I3>(L, count);
  }
}

void check_layout(const pgo::Layout& L, const std::vector<Region>& R) {
  const int n = (int)R.size();
  int64_t last_end = 0;
  for (int i = 0; i < n; ++i) {
    CHECK(R[i].offset % R[i].align == 0);
    CHECK(R[i].offset >= last_end);            // in call order, disjoint from everything before
    CHECK(R[i].offset < last_end + R[i].align);   // ... and no further than its alignment asks
    if (R[i].count) last_end = R[i].end;
  }
  CHECK(L.bytes() % 16 == 0 && L.bytes() >= last_end && L.bytes() < last_end + 16);
  // a run [a.offset, b.end()) holds the regions from a to b and no byte of another
  for (int a = 0; a < n; ++a)
    for (int b = a; b < n; ++b) {
      const int64_t lo = R[a].offset, hi = R[b].end;
      CHECK(hi - lo >= 0);
      for (int k = 0; k < n; ++k) {
        if (!R[k].count) continue;
        if (k >= a && k <= b) CHECK(R[k].offset >= lo && R[k].end <= hi);
        else CHECK(R[k].end <= lo || R[k].offset >= hi);
      }
    }
  // exactly bytes(): every element written, then every element read back
  void* base = malloc((size_t)L.bytes());
  CHECK(base != nullptr || L.bytes() == 0);
  for (int i = 0; i < n; ++i) R[i].write(base, R[i].offset, R[i].count, i);
  for (int i = 0; i < n; ++i) CHECK(R[i].read(base, R[i].offset, R[i].count, i));
  free(base);
}

int mixed_layouts() {
  const int64_t counts[] = {0, 1, 3, 15, 16, 17};
  int n_layouts = 0;
  for (int t0 = 0; t0 < N_TYPES; ++t0)         // the types rotated ...
    for (int step = 1; step <= 5; step += 4)   // ... forwards and backwards ...
      for (int c0 = 0; c0 < 6; ++c0)           // ... against the counts rotated, forwards and backwards
        for (int cstep = 1; cstep <= 5; cstep += 4) {
          pgo::Layout L, dense;
          std::vector<Region> R, D;
          for (int i = 0; i < N_TYPES; ++i) {
            const int type = (t0 + step * i) % N_TYPES;
            const int64_t count = counts[(c0 + cstep * i) % 6];
            R.push_back(add_type(&L, type, count));
            if (count) D.push_back(add_type(&dense, type, count));
          }
          check_layout(L, R);
          // the empty span cost nothing: the other regions lie where they lie without it
          CHECK(L.bytes() == dense.bytes());
          size_t d = 0;
          for (const Region& r : R)
            if (r.count) CHECK(r.offset == D[d++].offset);
          ++n_layouts;
        }
  {   // the same type twice in a row, and nothing at all
    pgo::Layout L, none;
    std::vector<Region> R;
    for (int64_t c : counts) R.push_back(add<I3>(&L, c));
    for (int64_t c : counts) R.push_back(add<uint8_t>(&L, c));
    check_layout(L, R);
    CHECK(none.bytes() == 0);
    check_layout(none, {});
    n_layouts += 2;
  }
  return n_layouts;
}

// pgo_loop_support's work buffer -- statistics | partials [4][nc] | q [n_sel] | records [E] | counts [3 n_sel] -- at
// E = n_sel = nc = 1: the counts lie behind ONE 24-byte record
void loop_support_work() {
  static_assert(sizeof(pgo_loop_support_record) == 24, "the record the case is about");
  const int64_t E = 1, n_sel = 1, nc = 1;
  pgo::Layout L;
  std::vector<Region> R;
  R.push_back(add<pgo_loop_support_stats>(&L, 1));
  R.push_back(add<double>(&L, 4 * nc));
  R.push_back(add<double>(&L, n_sel));
  R.push_back(add<pgo_loop_support_record>(&L, E));
  R.push_back(add<int32_t>(&L, 3 * n_sel));
  check_layout(L, R);
  CHECK(R[4].offset >= R[3].offset + 24 && L.bytes() >= R[4].offset + 12);
  // typed, as the call addresses it
  const pgo::Span<pgo_loop_support_record> out{R[3].offset, E};
  const pgo::Span<int32_t> cnt{R[4].offset, 3 * n_sel};
  const pgo::Span<pgo_loop_support_stats> stats{R[0].offset, 1};
  void* base = malloc((size_t)L.bytes());
  CHECK(base != nullptr);
  stats.in(base)->n_pairs_total = 1234567890123LL;
  out.in(base)[0].q_min = 0.25;
  out.in(base)[0].best = -1;
  for (int k = 0; k < 3; ++k) cnt.in(base)[k] = 7 + k;
  const void* cbase = base;
  CHECK(stats.in(cbase)->n_pairs_total == 1234567890123LL && out.in(cbase)[0].q_min == 0.25 && out.in(cbase)[0].best == -1);
  CHECK(cnt.in(cbase)[0] == 7 && cnt.in(cbase)[2] == 9);
  free(base);
  CHECK(pgo::run_bytes(out, cnt) == cnt.end() - out.offset);
}
}  // namespace

int main() {
  const int n_layouts = mixed_layouts();
  loop_support_work();
  printf("scratch ok: %d layouts, %ld checks\n", n_layouts, n_checks);
  return 0;
}
