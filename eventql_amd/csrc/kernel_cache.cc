// kernel_cache.cc -- hiprtc compilation of the generated kernels for gfx950, cached in
// memory per context and on disk by the digest of the source.
#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <mutex>
#include "runtime.h"
#include "sha1.h"

namespace evql {

static std::string g_cache_dir;
static bool g_cache_dir_set = false;

// Default place of the on-disk kernel cache: `_kcache` next to this shared library (the
// directory the python package points evql_set_kernel_cache_dir at too), so that every
// host of the library -- the adapter inside evqld, the probe, python -- shares the
// compiled plan kernels.  evql_set_kernel_cache_dir("") switches the disk cache off.
static const std::string& cache_dir() {
  if (!g_cache_dir_set) {
    g_cache_dir_set = true;
    Dl_info info;
    if (dladdr(reinterpret_cast<const void*>(&cache_dir), &info) && info.dli_fname) {
      std::string path = info.dli_fname;
      const size_t slash = path.rfind('/');
      g_cache_dir = (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/_kcache";
    }
  }
  return g_cache_dir;
}

void set_cache_dir(const std::string& d) {
  g_cache_dir = d;
  g_cache_dir_set = true;
}

static std::string hex_digest(const std::string& s) {
  Sha1Digest d = sha1(s.data(), s.size());
  char b[41];
  for (int i = 0; i < 20; ++i) snprintf(b + 2 * i, 3, "%02x", d.bytes[i]);
  return std::string(b, 40);
}

// ---------------------------------------------------------------------------
// kernel compilation (hiprtc, gfx950) with an in-memory and an on-disk cache
// ---------------------------------------------------------------------------
static const char* kCompileOptions[] = {"--offload-arch=gfx950", "-O3", "-munsafe-fp-atomics",
                                        "-ffp-contract=off", "-std=c++17"};

// an ELF header and, where it can be checked cheaply, a section header table inside
// the file: what a complete code object of the cache looks like
static bool plausible_code_object(const std::vector<char>& c) {
  if (c.size() < 64 || memcmp(c.data(), "\x7f" "ELF", 4) != 0) return false;
  uint64_t shoff;
  uint16_t shentsize, shnum;
  memcpy(&shoff, c.data() + 0x28, 8);
  memcpy(&shentsize, c.data() + 0x3a, 2);
  memcpy(&shnum, c.data() + 0x3c, 2);
  return shoff <= c.size() && uint64_t(shentsize) * shnum <= c.size() - shoff;
}

// process-wide counters: compilations outside any context (evql_compile_only)
static std::mutex g_stats_mutex;
static KernelCacheStats g_stats;

KernelCacheStats process_kernel_cache_stats() {
  std::lock_guard<std::mutex> lock(g_stats_mutex);
  return g_stats;
}

namespace {
// bumps `stats`, or the process-wide counters under their lock
struct StatsRef {
  KernelCacheStats* stats;
  template <typename F>
  void bump(F f) {
    if (stats) {
      f(*stats);
    } else {
      std::lock_guard<std::mutex> lock(g_stats_mutex);
      f(g_stats);
    }
  }
};
}  // namespace

Status compile_to_code_object(const std::string& source, std::vector<char>* code, bool use_cache,
                              KernelCacheStats* stats) {
  StatsRef sr{stats};
  const std::string full = std::string(device_library_source()) + "\n" + source;
  std::string key = hex_digest(full);
  std::string cache_file;
  const std::string& dir = cache_dir();
  if (!dir.empty()) {
    cache_file = dir + "/" + key + ".hsaco";
    std::ifstream f(cache_file, std::ios::binary);
    if (f && use_cache) {
      code->assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
      if (plausible_code_object(*code)) {
        sr.bump([](KernelCacheStats& k) { k.disk_hits += 1; });
        return Status();
      }
      code->clear();
    }
  }
  const auto t0 = std::chrono::steady_clock::now();
  hiprtcProgram prog;
  if (hiprtcCreateProgram(&prog, full.c_str(), "evql_fused.hip", 0, nullptr, nullptr) !=
      HIPRTC_SUCCESS) {
    return Status::error(EVQL_EDEVICE, "hiprtcCreateProgram failed");
  }
  hiprtcResult rc = hiprtcCompileProgram(
      prog, int(sizeof(kCompileOptions) / sizeof(kCompileOptions[0])), kCompileOptions);
  if (rc != HIPRTC_SUCCESS) {
    size_t ls = 0;
    hiprtcGetProgramLogSize(prog, &ls);
    std::string log(ls, '\0');
    if (ls) hiprtcGetProgramLog(prog, &log[0]);
    hiprtcDestroyProgram(&prog);
    return Status::error(EVQL_EDEVICE, "kernel compilation failed: " + log);
  }
  size_t cs = 0;
  hiprtcGetCodeSize(prog, &cs);
  code->resize(cs);
  hiprtcGetCode(prog, code->data());
  hiprtcDestroyProgram(&prog);
  const double ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  sr.bump([ms](KernelCacheStats& k) {
    k.compiles += 1;
    k.compile_ms += ms;
  });
  if (!cache_file.empty()) {
    mkdir(dir.c_str(), 0755);
    // (several processes -- one per GPU -- compile the same plan at the same time: each
    // writes a file of its own and renames it into place)
    static std::atomic<unsigned> serial{0};
    const std::string tmp = cache_file + "." + std::to_string(long(getpid())) + "." +
                            std::to_string(serial.fetch_add(1)) + ".tmp";
    std::ofstream f(tmp, std::ios::binary);
    f.write(code->data(), std::streamsize(code->size()));
    f.close();
    if (!f || rename(tmp.c_str(), cache_file.c_str()) != 0) remove(tmp.c_str());
  }
  return Status();
}

Status compile_kernel(evql_ctx* ctx, const std::string& source, Module* out, bool load_module) {
  const std::string key = hex_digest(source);
  if (ctx) {
    auto it = ctx->modules.find(key);
    if (it != ctx->modules.end()) {
      *out = it->second;
      ctx->kstats.memory_hits += 1;
      return Status();
    }
  }
  KernelCacheStats* stats = ctx ? &ctx->kstats : nullptr;
  std::vector<char> code;
  Status st = compile_to_code_object(source, &code, true, stats);
  if (!st.ok()) return st;
  out->code_size = code.size();
  if (load_module) {
    if (hipModuleLoadData(&out->mod, code.data()) != hipSuccess) {
      // a damaged cache file: compile again (and replace it)
      (void) hipGetLastError();
      st = compile_to_code_object(source, &code, false, stats);
      if (!st.ok()) return st;
      out->code_size = code.size();
      HIP_TRY(hipModuleLoadData(&out->mod, code.data()));
    }
    if (source.find("evql_scan_emit") != std::string::npos) {  // a bare scan
      HIP_TRY(hipModuleGetFunction(&out->fn_scan_count, out->mod, "evql_scan_count"));
      HIP_TRY(hipModuleGetFunction(&out->fn_scan_emit, out->mod, "evql_scan_emit"));
    } else {
      HIP_TRY(hipModuleGetFunction(&out->fn, out->mod, "evql_scan_agg"));
    }
    if (source.find("evql_part_aggregate") != std::string::npos) {
      out->fn_count = nullptr;  // (absent from the fused form, KernelPlan::part_fused)
      if (source.find("evql_part_count(") != std::string::npos) {
        HIP_TRY(hipModuleGetFunction(&out->fn_count, out->mod, "evql_part_count"));
      }
      HIP_TRY(hipModuleGetFunction(&out->fn_scatter, out->mod, "evql_part_scatter"));
      HIP_TRY(hipModuleGetFunction(&out->fn_aggregate, out->mod, "evql_part_aggregate"));
      if (source.find("evql_part_refine") != std::string::npos) {
        HIP_TRY(hipModuleGetFunction(&out->fn_refine, out->mod, "evql_part_refine"));
      }
    }
    if (source.find("evql_where_rows") != std::string::npos) {
      HIP_TRY(hipModuleGetFunction(&out->fn_where, out->mod, "evql_where_rows"));
    }
    if (ctx) ctx->modules[key] = *out;
  }
  return Status();
}

}  // namespace evql
