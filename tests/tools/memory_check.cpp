// memory_check.cpp -- mn_memory.h on the host, with allocators that hand out host memory, know every live pointer and
// fail on demand (tests/test_memory.py builds and runs it; it is its own program, so the sanitizers can build it too).
// The schedule mirrors the library's lifetimes: base, record and first-use groups; the record group swapped for a
// larger one; a carved workspace grown twice; batch arrays grown; everything freed.  It runs clean once, then once for
// every k with the k-th allocation failing.  After a failure, and at the end of every run:
//   - the registry's count equals the bytes of the live buffers that count;
//   - a field is null or holds a live pointer, each live pointer is held by one field, a group is whole or absent;
//   - `cap` / `batch_cap` / the workspace's capacity describe what is there;
//   - a free is of a live pointer of the right kind (the allocators see to that), and after free_all nothing is live.
// Exit status 0 and "ok ..." on stdout, or 1 and one line on stderr at the first violation.
#include <map>
#include <stdio.h>
#include <stdlib.h>

#include "../../mergenet_amd/csrc/mn_memory.h"

static char g_when[64] = "start";      // where the schedule stands, for the message
static void fail(const char* what, long long a = 0, long long b = 0) {
  fprintf(stderr, "memory_check: %s: %s (%lld, %lld)\n", g_when, what, a, b);
  exit(1);
}

// ---- allocators ---------------------------------------------------------------------------------------------
static std::map<void*, size_t> g_live[2];     // by MnMemKind: pointer -> bytes
static int g_allocs, g_fail_at;               // g_fail_at = k > 0: the k-th allocation fails

template <int KIND>
static int test_alloc(void** p, size_t bytes) {
  if (++g_allocs == g_fail_at) return 1;
  *p = malloc(bytes ? bytes : 1);
  if (!*p) fail("host malloc failed");
  g_live[KIND][*p] = bytes;
  return 0;
}
template <int KIND>
static void test_free(void* p) {
  if (!g_live[KIND].erase(p)) fail(g_live[1 - KIND].count(p) ? "free with the other kind's function" : "double free or free of an unknown pointer");
  free(p);
}

// ---- a context in the library's shape -------------------------------------------------------------------------
struct Ctx {
  MnMemory mem;
  int *base_a; double* base_b; char* h_stat;                       // base: two counted, one pinned
  int *rec_key, *rec_S, *rec_st; size_t cap;                       // records
  char *scratch_a, *scratch_b;                                     // first use
  struct Work { void* block; char* hs; int* rec; double* lp; long long* h_ctl; size_t n; } w;   // carved workspace
  struct Keep { int* d_P; int* d_X; int batch_cap; int extra; } k; // what outlives a regrow
};

static const size_t AL = 4096;

static int set_records(Ctx* c, size_t cap) {
  c->mem.free_group(MN_MEM_RECORDS);
  c->cap = 0;
  int rc = c->mem.alloc(&c->rec_key, cap * sizeof(int), MN_MEM_RECORDS, MN_MEM_DEVICE, true);
  if (rc == MN_OK) rc = c->mem.alloc(&c->rec_S, cap * sizeof(int), MN_MEM_RECORDS, MN_MEM_DEVICE, true);
  if (rc == MN_OK) rc = c->mem.alloc(&c->rec_st, cap * sizeof(int), MN_MEM_RECORDS, MN_MEM_DEVICE, true);
  if (rc != MN_OK) { c->mem.free_group(MN_MEM_RECORDS); return rc; }
  c->cap = cap;
  return MN_OK;
}

static size_t work_arrays(Ctx::Work& w, void* block, size_t n) {
  MnCarver k(block, AL);
  k.carve(w.hs, 3 * n + 1); k.carve(w.rec, n); k.carve(w.lp, n + 5);
  return k.off;
}

static int work_ensure(Ctx* c, size_t n) {
  if (c->w.n >= n) return MN_OK;
  c->mem.free_group(MN_MEM_EXACT);
  c->w = Ctx::Work();
  int rc = c->mem.alloc(&c->w.block, work_arrays(c->w, nullptr, n), MN_MEM_EXACT, MN_MEM_DEVICE, true);
  if (rc == MN_OK) rc = c->mem.alloc(&c->w.h_ctl, 128, MN_MEM_EXACT, MN_MEM_PINNED, false);
  if (rc != MN_OK) { c->mem.free_group(MN_MEM_EXACT); c->w = Ctx::Work(); return rc; }
  work_arrays(c->w, c->w.block, n);
  c->w.n = n;
  return MN_OK;
}

static int batch_ensure(Ctx* c, int n) {
  if (c->k.batch_cap >= n) return MN_OK;
  c->mem.free_group(MN_MEM_EXACT_BATCH);
  c->k.batch_cap = 0;
  int rc = c->mem.alloc(&c->k.d_P, n * sizeof(int), MN_MEM_EXACT_BATCH, MN_MEM_DEVICE, false);
  if (rc == MN_OK) rc = c->mem.alloc(&c->k.d_X, n * sizeof(int), MN_MEM_EXACT_BATCH, MN_MEM_DEVICE, false);
  if (rc != MN_OK) { c->mem.free_group(MN_MEM_EXACT_BATCH); return rc; }
  c->k.batch_cap = n;
  return MN_OK;
}

#define TRY(expr) do { const int rc_ = (expr); if (rc_ != MN_OK) return rc_; } while (0)

static int schedule(Ctx* c) {
  TRY(c->mem.alloc(&c->base_a, 1000, MN_MEM_BASE, MN_MEM_DEVICE, true));
  TRY(c->mem.alloc(&c->base_b, 777, MN_MEM_BASE, MN_MEM_DEVICE, true));
  TRY(c->mem.alloc(&c->h_stat, 144, MN_MEM_BASE, MN_MEM_PINNED, false));
  TRY(set_records(c, 100));
  TRY(c->mem.alloc(&c->scratch_a, 64, MN_MEM_SCRATCH, MN_MEM_DEVICE, true));
  TRY(c->mem.alloc(&c->scratch_b, 65, MN_MEM_SCRATCH, MN_MEM_DEVICE, true));
  TRY(set_records(c, 5000));
  c->k.extra = 7;
  TRY(work_ensure(c, 1000));
  TRY(work_ensure(c, 3000));
  TRY(work_ensure(c, 2000));                // (fits: nothing happens)
  TRY(batch_ensure(c, 2));
  TRY(batch_ensure(c, 5));
  return MN_OK;
}

// ---- the invariants -----------------------------------------------------------------------------------------------
struct Field { void* p; int kind, group; bool counted; };

// `destroyed`: after free_all, when every field must be null (the capacities then describe nothing: the library frees the context)
static void check(const Ctx* c, bool destroyed = false) {
  const Field f[] = {
      {c->base_a, MN_MEM_DEVICE, MN_MEM_BASE, true}, {c->base_b, MN_MEM_DEVICE, MN_MEM_BASE, true},
      {c->h_stat, MN_MEM_PINNED, MN_MEM_BASE, false},
      {c->rec_key, MN_MEM_DEVICE, MN_MEM_RECORDS, true}, {c->rec_S, MN_MEM_DEVICE, MN_MEM_RECORDS, true},
      {c->rec_st, MN_MEM_DEVICE, MN_MEM_RECORDS, true},
      {c->scratch_a, MN_MEM_DEVICE, MN_MEM_SCRATCH, true}, {c->scratch_b, MN_MEM_DEVICE, MN_MEM_SCRATCH, true},
      {c->w.block, MN_MEM_DEVICE, MN_MEM_EXACT, true}, {c->w.h_ctl, MN_MEM_PINNED, MN_MEM_EXACT, false},
      {c->k.d_P, MN_MEM_DEVICE, MN_MEM_EXACT_BATCH, false}, {c->k.d_X, MN_MEM_DEVICE, MN_MEM_EXACT_BATCH, false}};
  size_t counted = 0, held = 0;
  int present[16] = {0}, absent[16] = {0};
  for (const Field& x : f) {
    if (!x.p) { absent[x.group]++; continue; }
    present[x.group]++;
    held++;
    const auto it = g_live[x.kind].find(x.p);
    if (it == g_live[x.kind].end()) { fail("a field holds a pointer that is not live", x.group); }
    if (x.counted) counted += it->second;
  }
  const size_t live = g_live[0].size() + g_live[1].size();
  if (held != live) { fail("live buffers that no field holds (or one held twice)", (long long)live, (long long)held); }
  if ((size_t)c->mem.n != live) { fail("registry entries and live buffers differ", c->mem.n, (long long)live); }
  if (c->mem.counted != counted) { fail("counted bytes are not the sum of the live counted buffers", (long long)c->mem.counted, (long long)counted); }
  if (destroyed) {
    if (held) fail("a field is not null after free_all", (long long)held);
    return;
  }
  for (int g : {MN_MEM_RECORDS, MN_MEM_EXACT, MN_MEM_EXACT_BATCH})
    if (present[g] && absent[g]) { fail("a group is there in part", g); }
  if ((c->cap != 0) != (present[MN_MEM_RECORDS] != 0)) { fail("cap describes record lists that are not there", (long long)c->cap); }
  if ((c->k.batch_cap != 0) != (present[MN_MEM_EXACT_BATCH] != 0)) { fail("batch_cap describes arrays that are not there", c->k.batch_cap); }
  if ((c->w.n != 0) != (present[MN_MEM_EXACT] != 0) || (!c->w.block && (c->w.hs || c->w.rec || c->w.lp))) {
    fail("the workspace's capacity or arrays describe a block that is not there", (long long)c->w.n);
  }
  if (c->cap && g_live[0][c->rec_key] != c->cap * sizeof(int)) { fail("cap is not the lists' size", (long long)c->cap); }
}

static Ctx* new_ctx() {
  Ctx* c = static_cast<Ctx*>(calloc(1, sizeof(Ctx)));
  if (!c) fail("host calloc failed");
  c->mem.alloc_fn[MN_MEM_DEVICE] = test_alloc<MN_MEM_DEVICE>; c->mem.free_fn[MN_MEM_DEVICE] = test_free<MN_MEM_DEVICE>;
  c->mem.alloc_fn[MN_MEM_PINNED] = test_alloc<MN_MEM_PINNED>; c->mem.free_fn[MN_MEM_PINNED] = test_free<MN_MEM_PINNED>;
  return c;
}

// One run of the schedule with the k-th allocation failing (0: none); returns the allocations it made.
static int run(int k) {
  snprintf(g_when, sizeof(g_when), k ? "allocation %d failed" : "clean run", k);
  Ctx* c = new_ctx();
  g_allocs = 0; g_fail_at = k;
  const int rc = schedule(c);
  g_fail_at = 0;
  if (rc != (k ? MN_ERR_NO_DEVICE : MN_OK)) fail("the schedule's status is not what the failure asks for", rc, k);
  check(c);
  if (k == 0) {
    if (c->cap != 5000 || c->w.n != 3000 || c->k.batch_cap != 5 || c->k.extra != 7) fail("the clean run did not end where it should");
    // the carved arrays of the last workspace: inside the block, in order, apart
    const char* b = static_cast<const char*>(c->w.block);
    if (c->w.hs != b || (const char*)c->w.rec != b + 3 * AL || (const char*)c->w.lp != b + 6 * AL ||
        g_live[0][c->w.block] != 12 * AL)
      fail("the carved workspace is not 3 + 3 + 6 pages");
    if (c->mem.counted != 1000 + 777 + 3 * 5000 * sizeof(int) + 64 + 65 + 12 * AL) fail("the clean run's counted bytes", (long long)c->mem.counted);
  }
  const int allocs = g_allocs;
  c->mem.free_all();
  check(c, true);
  if (!g_live[0].empty() || !g_live[1].empty() || c->mem.counted != 0 || c->mem.n != 0)
    fail("something is live or counted after free_all", (long long)(g_live[0].size() + g_live[1].size()), (long long)c->mem.counted);
  c->mem.free_all();                          // (a second one finds nothing to free)
  free(c);
  return allocs;
}

// The entry array is full: MN_ERR_INTERNAL, the field null, nothing allocated.
static void capacity_case() {
  snprintf(g_when, sizeof(g_when), "capacity case");
  Ctx* c = new_ctx();
  static char* many[MN_MEM_ENTRIES + 1];
  g_allocs = 0;
  for (int i = 0; i < MN_MEM_ENTRIES; i++)
    if (c->mem.alloc(&many[i], 8, MN_MEM_SCRATCH, MN_MEM_DEVICE, true) != MN_OK) fail("an allocation within the capacity failed", i);
  many[MN_MEM_ENTRIES] = reinterpret_cast<char*>(c);
  if (c->mem.alloc(&many[MN_MEM_ENTRIES], 8, MN_MEM_SCRATCH, MN_MEM_DEVICE, true) != MN_ERR_INTERNAL || many[MN_MEM_ENTRIES] ||
      g_allocs != MN_MEM_ENTRIES || c->mem.counted != 8 * (size_t)MN_MEM_ENTRIES)
    fail("a full registry must refuse with MN_ERR_INTERNAL and leave the field null");
  c->mem.free_group(MN_MEM_SCRATCH);
  for (int i = 0; i < MN_MEM_ENTRIES; i++)
    if (many[i]) fail("a field of a freed group is not null", i);
  if (!g_live[0].empty() || c->mem.counted != 0) fail("something is live after the capacity case");
  free(c);
}

// Three arrays whose sizes are no multiples of the alignment: 5 chars, 3 ints, 7 doubles at 16 bytes -> 0, 16, 32; 96 in all.
static void carver_case() {
  snprintf(g_when, sizeof(g_when), "carver case");
  char* a = nullptr; int* b = nullptr; double* d = nullptr;
  auto arrays = [&](void* base) { MnCarver k(base, 16); k.carve(a, 5); k.carve(b, 3); k.carve(d, 7); return k.off; };
  const size_t total = arrays(nullptr);
  if (a || b || d) fail("the sizing pass set a field");
  if (total != 96) fail("carver: total of the sizing pass", (long long)total, 96);
  char* block = static_cast<char*>(aligned_alloc(32, total));      // (96 = 3 * 32)
  if (!block) fail("host aligned_alloc failed");
  if (arrays(block) != total) fail("carver: the two passes disagree on the total");
  const char* at[4] = {a, reinterpret_cast<char*>(b), reinterpret_cast<char*>(d), block + total};
  const size_t size[3] = {5 * sizeof(char), 3 * sizeof(int), 7 * sizeof(double)};
  if (at[0] != block) fail("carver: the first array is not at the base");
  for (int i = 0; i < 3; i++) {
    if ((at[i] - block) % 16 != 0) fail("carver: an array is not aligned", i, at[i] - block);
    if (at[i] + size[i] > at[i + 1]) fail("carver: arrays overlap (or the last one leaves the block)", i);
  }
  a[4] = 1; b[2] = 2; d[6] = 3.0;             // (the last element of each: the sanitizers watch the block's end)
  free(block);
}

int main() {
  const int allocs = run(0);
  if (allocs != 19) fail("the clean run's number of allocations", allocs, 19);
  for (int k = 1; k <= allocs; k++) run(k);
  capacity_case();
  carver_case();
  printf("ok: clean run of %d allocations, %d runs with one failing, capacity, carver\n", allocs, allocs);
  return 0;
}
