// TEST INFRASTRUCTURE — runtime of the host-only HIP stand-in (see hip/hip_runtime.h).
#include <hip/hip_runtime.h>

#include <sys/mman.h>

#include <atomic>
#include <map>
#include <mutex>

namespace hipmock {

uint3_t g_threadIdx, g_blockIdx;
dim3 g_blockDim, g_gridDim;
double g_xchg_d[1024];
long long g_xchg_i[1024];

namespace {

constexpr size_t kStackBytes = 256 * 1024;
constexpr int kMaxThreads = 1024;

extern "C" void hipmock_ctx_switch(void** from_sp, void* to_sp);
asm(R"(
.text
.globl hipmock_ctx_switch
.type hipmock_ctx_switch,@function
hipmock_ctx_switch:
  pushq %rbp
  pushq %rbx
  pushq %r12
  pushq %r13
  pushq %r14
  pushq %r15
  movq %rsp, (%rdi)
  movq %rsi, %rsp
  popq %r15
  popq %r14
  popq %r13
  popq %r12
  popq %rbx
  popq %rbp
  ret
.size hipmock_ctx_switch,.-hipmock_ctx_switch
)");

struct Fiber {
  void* sp = nullptr;
  char* stack = nullptr;
  bool done = true;
  uint3_t tid;
};

Fiber g_fibers[kMaxThreads];
void* g_sched_sp = nullptr;
int g_current = -1;
const std::function<void()>* g_body = nullptr;

void fiber_entry() {
  (*g_body)();
  g_fibers[g_current].done = true;
  hipmock_ctx_switch(&g_fibers[g_current].sp, g_sched_sp);
  abort();  // a finished fiber is never resumed
}

void prepare(Fiber& f) {
  if (!f.stack) {
    f.stack = (char*)mmap(nullptr, kStackBytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (f.stack == (char*)MAP_FAILED) {
      fprintf(stderr, "hipmock: cannot allocate a fiber stack\n");
      abort();
    }
  }
  uintptr_t top = ((uintptr_t)(f.stack + kStackBytes)) & ~(uintptr_t)15;
  void** sp = (void**)(top - 64);
  for (int i = 0; i < 6; ++i) sp[i] = nullptr;
  sp[6] = (void*)&fiber_entry;
  sp[7] = nullptr;
  f.sp = sp;
  f.done = false;
}

}  // namespace

int linear_tid() { return (int)(g_threadIdx.x + g_blockDim.x * (g_threadIdx.y + g_blockDim.y * g_threadIdx.z)); }

void yield_barrier() { hipmock_ctx_switch(&g_fibers[g_current].sp, g_sched_sp); }

void run_grid(dim3 grid, dim3 block, const std::function<void()>& body) {
  const int nthreads = (int)(block.x * block.y * block.z);
  if (nthreads > kMaxThreads || nthreads <= 0) {
    fprintf(stderr, "hipmock: bad block size %d\n", nthreads);
    abort();
  }
  g_blockDim = block;
  g_gridDim = grid;
  g_body = &body;
  for (unsigned bz = 0; bz < grid.z; ++bz)
    for (unsigned by = 0; by < grid.y; ++by)
      for (unsigned bx = 0; bx < grid.x; ++bx) {
        g_blockIdx = uint3_t{bx, by, bz};
        int t = 0;
        for (unsigned tz = 0; tz < block.z; ++tz)
          for (unsigned ty = 0; ty < block.y; ++ty)
            for (unsigned tx = 0; tx < block.x; ++tx, ++t) {
              prepare(g_fibers[t]);
              g_fibers[t].tid = uint3_t{tx, ty, tz};
            }
        int live = nthreads;
        while (live > 0) {
          live = 0;
          for (int i = 0; i < nthreads; ++i) {
            Fiber& f = g_fibers[i];
            if (f.done) continue;
            g_current = i;
            g_threadIdx = f.tid;
            hipmock_ctx_switch(&g_sched_sp, f.sp);
            if (!f.done) ++live;
          }
        }
      }
  g_body = nullptr;
}

}  // namespace hipmock

// ---- guard mode (tests/test_memory_contract.py) ---------------------------------------------------------------------
// Off (the default): hipMalloc is malloc, as ever.  On (hipmock_guard_enable(1), at run time, through ctypes): every new
// block lies between two red zones of kRedZoneBytes holding kRedZoneByte, its payload starts as kPayloadByte (0xFF: a NaN
// as a double, -1 as an integer: what a kernel reads that relies on fresh device memory being anything in particular),
// and hipFree, hipmock_guard_check_all and the host-initiated copies / memsets record what they find, never abort.
// Every live block is in g_blocks with its kind, so a block of either kind is freed the way it was allocated whatever
// the mode is by then.
namespace {

constexpr size_t kRedZoneBytes = 64 * 1024;  // >= two rows of the widest 2-D level of the tests (256 doubles = 2 KiB a row)
constexpr unsigned char kRedZoneByte = 0xA5;
constexpr unsigned char kPayloadByte = 0xFF;  // fresh and freed payloads

struct Block {
  size_t bytes;
  bool guarded;
  unsigned long long seq;
};

std::mutex g_guard_mu;
std::map<char*, Block> g_blocks;  // payload start -> block, both kinds
std::atomic<bool> g_guard{false};  // (read by range_ok and hipmock_guard_enabled without the mutex)
unsigned long long g_alloc_seq = 0;
std::vector<hipmock_violation> g_violations;

void record(int kind, int side, const Block* b, long long offset, size_t length) {
  g_violations.push_back(hipmock_violation{kind, side, b ? (unsigned long long)b->bytes : 0ULL, offset, b ? b->seq : 0ULL, (unsigned long long)length});
}

// both red zones of a guarded block: the first bad byte of each side is recorded and the zone repaired (one record per damage)
void check_zones(char* payload, const Block& b) {
  char* zone[2] = {payload - kRedZoneBytes, payload + b.bytes};
  for (int side = 0; side < 2; ++side)
    for (size_t i = 0; i < kRedZoneBytes; ++i)
      if ((unsigned char)zone[side][i] != kRedZoneByte) {
        record(HIPMOCK_VIOLATION_RED_ZONE, side, &b, (long long)(zone[side] + i - payload), 1);
        memset(zone[side], kRedZoneByte, kRedZoneBytes);
        break;
      }
}

// the live block whose payload or red zones hold p (null: none); start: its payload.  Caller holds g_guard_mu.
const Block* block_near(const char* p, const char** start) {
  auto above = g_blocks.upper_bound(const_cast<char*>(p));  // first payload that starts beyond p
  if (above != g_blocks.begin()) {
    auto below = std::prev(above);
    if (p < below->first + below->second.bytes + (below->second.guarded ? kRedZoneBytes : 0)) {
      *start = below->first;
      return &below->second;
    }
  }
  if (above != g_blocks.end() && above->second.guarded && p >= above->first - kRedZoneBytes) {
    *start = above->first;
    return &above->second;
  }
  return nullptr;
}

// a device-side range of a host-initiated copy or memset lies inside one live payload.  known_device = false (a side of
// hipMemcpyDefault, which names none): the side is a device side if it points into a live block or its red zones.
bool range_ok(const void* ptr, size_t bytes, bool known_device = true) {
  if (!g_guard.load()) return true;
  std::lock_guard<std::mutex> lock(g_guard_mu);
  const char* p = (const char*)ptr;
  const char* start = nullptr;
  const Block* near = block_near(p, &start);
  if (!near && !known_device) return true;  // host memory
  if (near && p >= start && p + bytes <= start + near->bytes) return true;
  record(HIPMOCK_VIOLATION_RANGE, near ? (p < start ? 0 : 1) : -1, near, near ? (long long)(p - start) : 0, bytes);
  return false;
}

// a side of a copy: checked as device memory (1), resolved by looking the pointer up (hipMemcpyDefault: 0), host (-1)
int device_side(hipMemcpyKind k, bool dst) {
  if (k == hipMemcpyHostToHost) return -1;
  if (k == hipMemcpyHostToDevice) return dst ? 1 : -1;
  if (k == hipMemcpyDeviceToHost) return dst ? -1 : 1;
  return k == hipMemcpyDeviceToDevice ? 1 : 0;
}

bool side_ok(hipMemcpyKind k, bool dst, const void* p, size_t bytes) {
  const int side = device_side(k, dst);
  return side < 0 || range_ok(p, bytes, side == 1);
}

}  // namespace

extern "C" {
void hipmock_guard_enable(int on) {
  g_guard.store(on != 0);
}
int hipmock_guard_enabled() { return g_guard.load() ? 1 : 0; }
int hipmock_guard_red_zone_bytes() { return (int)kRedZoneBytes; }
int hipmock_guard_live_blocks() {
  std::lock_guard<std::mutex> lock(g_guard_mu);
  int n = 0;
  for (auto& b : g_blocks) n += b.second.guarded ? 1 : 0;
  return n;
}
int hipmock_guard_check_all() {
  std::lock_guard<std::mutex> lock(g_guard_mu);
  for (auto& b : g_blocks)
    if (b.second.guarded) check_zones(b.first, b.second);
  return (int)g_violations.size();
}
int hipmock_guard_take(hipmock_violation* out, int capacity) {
  std::lock_guard<std::mutex> lock(g_guard_mu);
  const int total = (int)g_violations.size();
  for (int i = 0; i < total && i < capacity; ++i) out[i] = g_violations[i];
  g_violations.clear();
  return total;
}
}

hipError_t hipMalloc(void** p, size_t bytes) {
  if (bytes == 0) bytes = 1;
  std::lock_guard<std::mutex> lock(g_guard_mu);
  char* payload = nullptr;
  const bool guarded = g_guard.load();
  if (guarded) {
    char* raw = (char*)malloc(bytes + 2 * kRedZoneBytes);
    if (raw) {
      payload = raw + kRedZoneBytes;
      memset(raw, kRedZoneByte, kRedZoneBytes);
      memset(payload, kPayloadByte, bytes);
      memset(payload + bytes, kRedZoneByte, kRedZoneBytes);
    }
  } else {
    payload = (char*)malloc(bytes);
  }
  *p = payload;
  if (!payload) return hipErrorOutOfMemory;
  g_blocks[payload] = Block{bytes, guarded, ++g_alloc_seq};
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  if (!p) return hipSuccess;
  std::lock_guard<std::mutex> lock(g_guard_mu);
  auto it = g_blocks.find((char*)p);
  if (it == g_blocks.end()) {  // not a live block: freed already, an interior pointer, or never ours
    if (!g_guard.load()) {
      free(p);  // (mode off: free() as ever)
      return hipSuccess;
    }
    record(HIPMOCK_VIOLATION_BAD_FREE, -1, nullptr, 0, 1);
    return hipErrorInvalidValue;
  }
  const Block b = it->second;
  g_blocks.erase(it);
  if (!b.guarded) {
    free(p);
    return hipSuccess;
  }
  check_zones((char*)p, b);
  memset(p, kPayloadByte, b.bytes);  // a use after free reads NaN
  free((char*)p - kRedZoneBytes);
  return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind k) {
  if (bytes && (!side_ok(k, true, dst, bytes) || !side_ok(k, false, src, bytes))) return hipErrorInvalidValue;
  memmove(dst, src, bytes);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind k, hipStream_t) { return hipMemcpy(dst, src, bytes, k); }
hipError_t hipMemset(void* dst, int value, size_t bytes) {
  if (bytes && !range_ok(dst, bytes)) return hipErrorInvalidValue;
  memset(dst, value, bytes);
  return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t) { return hipMemset(dst, value, bytes); }
// the allocator for a ctypes caller (the C++ names above are mangled): the guard's own test plants its errors through these
extern "C" {
int hipmock_malloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
int hipmock_free(void* p) { return hipFree(p); }
int hipmock_memset(void* dst, int value, size_t bytes) { return hipMemset(dst, value, bytes); }
int hipmock_memcpy(void* dst, const void* src, size_t bytes, int kind) { return hipMemcpy(dst, src, bytes, (hipMemcpyKind)kind); }
}
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDevice(int* d) {
  *d = 0;
  return hipSuccess;
}
hipError_t hipGetDeviceCount(int* n) {
  *n = 1;
  return hipSuccess;
}
hipError_t hipGetDeviceProperties(hipDeviceProp_t* prop, int) {
  memset(prop, 0, sizeof(*prop));
  snprintf(prop->name, sizeof(prop->name), "hipmock CPU emulator");
  snprintf(prop->gcnArchName, sizeof(prop->gcnArchName), "cpu-fibers");
  prop->multiProcessorCount = 4;
  return hipSuccess;
}
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "success" : "hipmock error"; }
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipDeviceSynchronize() { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) {
  *e = new mock_event();
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) {
  e->t = std::chrono::steady_clock::now();
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  *ms = std::chrono::duration<float, std::milli>(b->t - a->t).count();
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
  delete e;
  return hipSuccess;
}
