// mn_memory.h -- the one owner of a context's memory.  Every buffer of mn_context is allocated INTO its field through
// the registry below, which remembers the field, the size and the group; a group is freed as a whole (its fields come
// back null), mn_destroy frees all of them, and mn_workspace_bytes is the registry's count.  Nothing else in the
// library calls an allocator or keeps a list of buffers.  Plain host C++ that g++ alone compiles: the allocators are
// the caller's (the library: hipMalloc / hipFree / hipHostMalloc / hipHostFree; tests/tools/memory_check.cpp: its own,
// which fail on demand and know every live pointer).
#pragma once
#include <stddef.h>
#include "../../include/mergenet_hip.h"

// Groups: buffers that live and die together.
enum MnMemGroup {
  MN_MEM_BASE,             // mn_create
  MN_MEM_RECORDS,          // record lists and record table (small at mn_create, full size for the general rounds)
  MN_MEM_FAST,             // what only the fast paths use
  MN_MEM_STAGING,          // device copies for the host-pointer entry points
  MN_MEM_SCRATCH,          // single buffers allocated where an entry point first needs them
  MN_MEM_EXACT,            // workspace of the exact engine (regrown for a larger image or a run that filled it)
  MN_MEM_EXACT_BATCH,      // ... its per-batch arrays
  MN_MEM_REFORDER,         // workspace of the reference-order loop
  MN_MEM_REFORDER_BATCH,   // ... its per-batch array
};
enum MnMemKind { MN_MEM_DEVICE, MN_MEM_PINNED };
#define MN_MEM_ENTRIES 96   // (a context registers 64 buffers when every path has run)

struct MnMemory {
  // by MnMemKind; alloc returns 0 and sets the pointer, or non-zero
  int (*alloc_fn[2])(void**, size_t);
  void (*free_fn[2])(void*);
  struct Entry { void** field; size_t bytes; int group, kind; bool counted; } entry[MN_MEM_ENTRIES];
  int n;
  size_t counted;          // bytes of the live entries that count toward mn_workspace_bytes

  // `bytes` into *field (which holds nothing yet).  Registered only when it succeeded: a failure leaves the field
  // null and the count as it was.
  template <typename T>
  int alloc(T** field, size_t bytes, int group, int kind, bool count) {
    *field = nullptr;
    if (n == MN_MEM_ENTRIES) return MN_ERR_INTERNAL;
    void* p = nullptr;
    if (alloc_fn[kind](&p, bytes) != 0) return MN_ERR_NO_DEVICE;
    *field = static_cast<T*>(p);
    entry[n++] = Entry{reinterpret_cast<void**>(field), bytes, group, kind, count};
    if (count) counted += bytes;
    return MN_OK;
  }
  // Releases the group's buffers, nulls their fields and takes back exactly what was counted for them.
  void free_group(int group, bool all = false) {
    int kept = 0;
    for (int i = 0; i < n; i++) {
      const Entry e = entry[i];
      if (!all && e.group != group) { entry[kept++] = e; continue; }
      if (*e.field) free_fn[e.kind](*e.field);
      *e.field = nullptr;
      if (e.counted) counted -= e.bytes;
    }
    n = kept;
  }
  void free_all() { free_group(0, true); }
};

// Arrays at aligned offsets of one block, listed ONCE by the caller in a function of the base: run with a null base it
// only sizes the block (`off` at the end), run with the block it also sets the fields.
struct MnCarver {
  char* base;
  size_t align, off;
  MnCarver(void* b, size_t a) : base(static_cast<char*>(b)), align(a), off(0) {}
  template <typename T>
  void carve(T*& field, size_t count) {
    if (base) field = reinterpret_cast<T*>(base + off);
    off += (count * sizeof(T) + align - 1) / align * align;
  }
};
