// Run-time compiled expression kernels for ZXP programs.
//
// The reference ships its constraint/FRI expressions as generated C++ compiled
// into the prover (src/starkpil/*/chelpers/*.step42ns.cpp, step52ns.cpp: one
// straight-line function per circuit).  This is the GPU equivalent: the
// compiled program is printed as one straight-line HIP kernel
// (csrc/zxp_jit_source.cpp) and compiled for gfx950 with hiprtc on first use;
// one compiled kernel serves every proof of a circuit (cached per process by
// source text, and on disk).  Here: hiprtc, the disk cache, the occupancy
// decisions, segments and the launch.
//
// Unsupported shapes (a program that reads a column it writes at a row shift
// it did not write first) return 1 and the caller runs the interpreter.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>
#include <utime.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "zkgpu_internal.hpp"
#include "zxp_segment.hpp"

#include <algorithm>
#include <atomic>
#include <functional>
#include <thread>

namespace zk {

namespace {

constexpr int JIT_THREADS = 256;

// kernel argument (the kernel head in csrc/zxp_jit_source.cpp declares the same layout)
struct JitParams {
    const uint64_t *const *cp;  // column base pointers (slot j)
    const uint64_t *kc;         // F_p / F_p^3 constants
    const uint32_t *kl;         // DOT limbs (unrolled terms)
    const JitTerm *zt;          // DOT column terms (looped)
    const uint64_t *xdiv, *xdivw, *zh, *tw_lo, *tw_hi;
    uint64_t x_start, rmask;
    uint32_t logdom, logomega, zmask;
    uint32_t nkl;  // limb words staged in LDS (0: read from p.kl)
    uint32_t one;  // always 1: the uniform branch that closes each code block (compile time)
};

struct Cache {
    std::mutex mu;
    std::unordered_map<std::string, hipFunction_t> fn;
};
Cache &cache()
{
    static Cache c;
    return c;
}

// grow-only device buffer for the per-launch tables (in_use: the event after
// the last kernels that read it)
char *jit_buf(size_t bytes, hipEvent_t in_use)
{
    static char *buf = nullptr;
    static size_t cap = 0;
    if (bytes > cap) {
        if (in_use) (void)hipEventSynchronize(in_use);
        if (buf) (void)hipFree(buf);
        buf = nullptr;
        cap = 0;
        if (hipMalloc((void **)&buf, bytes) != hipSuccess) return nullptr;
        cap = bytes;
    }
    return buf;
}

// hiprtc: source -> gfx950 code object (no GPU needed)
int rtc_compile(const std::string &src, std::vector<char> &code)
{
    hiprtcProgram prog;
    if (hiprtcCreateProgram(&prog, src.c_str(), "zxp_jit.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
        return set_error(ZKGPU_ERR_ARG, "zxp jit: hiprtcCreateProgram failed");
    // LDS-staged limb tables compile at -O2: the load/store vectorizer merges
    // each term's limb reads into 16+8-byte loads (-O1 does not run it).
    // Otherwise -O1 (-O2 is no faster there: the scheduler hoists more scalar
    // loads, e.g. step42ns without LDS 14.1 -> 16.7 ms).  Compile time is about
    // the same.
    const bool klds = src.find("#define ZKJIT_KL_LDS 1") != std::string::npos;
    const char *olev = klds ? "-O2" : "-O1";
    // The GCN scheduler's re-scheduling stages (unclustered high-pressure and
    // clustered low-occupancy) re-run the scheduler over every region and
    // doubled the compile time of the large programs; register pressure is
    // already bounded by the ZXP scheduler (csrc/zxp_compile.cpp), so they
    // are off for them.
    // Small programs keep them: there they lower register pressure (config-4
    // quotient 17.2 -> 15.2 ms, FRI polynomial 10.4 -> 9.1 ms at 2^23) and
    // cost little compile time.
    const bool resched = src.find("#define ZKJIT_SPLIT 1") == std::string::npos;
    std::vector<const char *> opts = {"--offload-arch=gfx950", olev, "-std=c++17"};
    if (!resched) {
        opts.push_back("-mllvm");
        opts.push_back("-amdgpu-disable-unclustered-high-rp-reschedule=1");
        opts.push_back("-mllvm");
        opts.push_back("-amdgpu-disable-clustered-low-occupancy-reschedule=1");
    }
    const hiprtcResult r = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
    if (r != HIPRTC_SUCCESS) {
        size_t ls = 0;
        hiprtcGetProgramLogSize(prog, &ls);
        std::string log(ls + 1, '\0');
        hiprtcGetProgramLog(prog, &log[0]);
        hiprtcDestroyProgram(&prog);
        return set_error(ZKGPU_ERR_ARG, "zxp jit: hiprtc compile failed: %.300s", log.c_str());
    }
    size_t cs = 0;
    hiprtcGetCodeSize(prog, &cs);
    code.resize(cs);
    hiprtcGetCode(prog, code.data());
    hiprtcDestroyProgram(&prog);
    return cs ? 0 : set_error(ZKGPU_ERR_ARG, "zxp jit: empty code object");
}

// On-disk code-object cache: a program's kernel depends only on its
// structure (the source text) and the compiler, so compiled objects are kept
// in ZKGPU_JIT_CACHE (default: <libzkgpu dir>/../jitcache, created on demand;
// "0" disables) under a hash of source + options + hiprtc version.  build()
// fills it ahead of time for the known circuits (the reference ships its
// expression code compiled, chelpers/*.cpp).
static std::string cache_dir()
{
    static const std::string dir = [] {
        const char *e = getenv("ZKGPU_JIT_CACHE");
        if (e) return std::string(strcmp(e, "0") ? e : "");
        Dl_info info;
        if (dladdr((void *)&cache_dir, &info) && info.dli_fname) {
            std::string so = info.dli_fname;
            const size_t sl = so.rfind('/');
            if (sl != std::string::npos) return so.substr(0, sl) + "/../jitcache";
        }
        return std::string();
    }();
    return dir;
}

static std::string cache_key(const std::string &src)
{
    int major = 0, minor = 0;
    hiprtcVersion(&major, &minor);
    uint64_t h1 = 1469598103934665603ULL, h2 = 0x9E3779B97F4A7C15ULL;
    auto mix = [&](const char *p, size_t n) {
        for (size_t i = 0; i < n; i++) {
            h1 = (h1 ^ (uint8_t)p[i]) * 1099511628211ULL;
            h2 = (h2 + (uint8_t)p[i]) * 0xBF58476D1CE4E5B9ULL;
            h2 ^= h2 >> 29;
        }
    };
    mix(src.data(), src.size());
    char opt[160];
    // ("opt- resched-": the compile options are a function of the source,
    // which is hashed above; the text keeps the keys of existing entries)
    snprintf(opt, sizeof(opt), "hiprtc%d.%d hip%d gfx950 opt- resched-", major, minor, (int)HIP_VERSION);
    mix(opt, strlen(opt));
    char key[64];
    snprintf(key, sizeof(key), "zxp_%016llx%016llx.co", (unsigned long long)h1, (unsigned long long)h2);
    return key;
}

// On-disk entry: "ZKJITCO2", u32 key length, key (cache_key: hash of source,
// options, hiprtc / HIP versions, target), u64 object length, object.  A file
// that does not carry this exact key and a complete ELF object is a miss.
static const char JIT_CO_MAGIC[8] = {'Z', 'K', 'J', 'I', 'T', 'C', 'O', '2'};

static bool cache_load(const std::string &src, std::vector<char> &code)
{
    const std::string dir = cache_dir();
    if (dir.empty()) return false;
    const std::string key = cache_key(src);
    FILE *f = fopen((dir + "/" + key).c_str(), "rb");
    if (!f) return false;
    char magic[8];
    uint32_t kn = 0;
    uint64_t n = 0;
    bool ok = fread(magic, 1, 8, f) == 8 && !memcmp(magic, JIT_CO_MAGIC, 8) && fread(&kn, 4, 1, f) == 1 &&
              kn == key.size();
    if (ok) {
        std::string k2(kn, '\0');
        ok = fread(&k2[0], 1, kn, f) == kn && k2 == key && fread(&n, 8, 1, f) == 1 && n > 4 && n < (1ULL << 32);
    }
    if (ok) {
        code.resize(n);
        ok = fread(code.data(), 1, n, f) == n && fgetc(f) == EOF && !memcmp(code.data(), "\x7f" "ELF", 4);
    }
    fclose(f);
    if (ok) utime((dir + "/" + key).c_str(), nullptr);  // in use: tools/jit_prebuild.py --prune keeps it
    return ok;
}

static void cache_store(const std::string &src, const std::vector<char> &code)
{
    const std::string dir = cache_dir();
    if (dir.empty()) return;
    mkdir(dir.c_str(), 0775);
    const std::string key = cache_key(src);
    const std::string path = dir + "/" + key, tmp = path + ".tmp" + std::to_string(getpid());
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return;
    const uint32_t kn = (uint32_t)key.size();
    const uint64_t n = code.size();
    const bool ok = fwrite(JIT_CO_MAGIC, 1, 8, f) == 8 && fwrite(&kn, 4, 1, f) == 1 && fwrite(key.data(), 1, kn, f) == kn &&
                    fwrite(&n, 8, 1, f) == 1 && fwrite(code.data(), 1, n, f) == n;
    fclose(f);
    if (ok) rename(tmp.c_str(), path.c_str());
    else unlink(tmp.c_str());
}

// source -> code object: the disk cache, else hiprtc (and fill the cache);
// *cached tells which
int code_object(const std::string &src, std::vector<char> &code, bool *cached = nullptr)
{
    if (cached) *cached = false;
    if (cache_load(src, code)) {
        if (cached) *cached = true;
        return 0;
    }
    int rc;
    static const bool log = getenv("ZKGPU_JIT_LOG") && atoi(getenv("ZKGPU_JIT_LOG"));
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = rtc_compile(src, code))) return rc;
    cache_store(src, code);
    if (log)  // cache misses (tools/jit_prebuild.py fills the cache ahead of time)
        fprintf(stderr, "[zkgpu jit] cache miss: %s compiled in %.1f s\n", cache_key(src).c_str(),
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}

// one kernel ready to launch: source and tables, compiled function
struct JitKernel : ZxpJitSource {
    hipFunction_t fn = nullptr;
    size_t off = 0, off_cp = 0, off_kc = 0, off_kl = 0, end = 0;  // table layout in the launch buffer
    bool klds = false;
    double bytes = 0;
};

// code objects of several sources (disk cache or hiprtc), compiled in
// parallel threads: the segments of a large program are independent
void objects_parallel(const std::vector<const std::string *> &srcs, std::vector<std::vector<char>> &code,
                      std::vector<int> &rcs, std::vector<uint8_t> *from_cache = nullptr)
{
    code.assign(srcs.size(), {});
    rcs.assign(srcs.size(), 0);
    if (from_cache) from_cache->assign(srcs.size(), 0);
    static const unsigned nthr = [] {
        const char *e = getenv("ZKGPU_ZXP_JIT_THREADS");
        const unsigned hc = std::max(1u, std::thread::hardware_concurrency());
        return e && atoi(e) > 0 ? (unsigned)atoi(e) : std::min(16u, hc);
    }();
    std::vector<std::thread> th;
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t j; (j = next++) < srcs.size();) {
            bool hit = false;
            rcs[j] = code_object(*srcs[j], code[j], &hit);
            if (from_cache) (*from_cache)[j] = hit;
        }
    };
    const unsigned n = std::min<unsigned>(nthr, (unsigned)srcs.size());
    for (unsigned t = 1; t < n; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
}

// code objects of several kernels: the ones not in this process's cache are
// found on disk or compiled by hiprtc, in parallel (the segments of a large
// program compile independently), then loaded
int compile_all(std::vector<JitKernel *> ks)
{
    Cache &c = cache();
    std::lock_guard<std::mutex> lk(c.mu);
    std::vector<JitKernel *> todo;
    for (JitKernel *k : ks) {
        auto it = c.fn.find(k->src);
        if (it != c.fn.end())
            k->fn = it->second;
        else if (std::find_if(todo.begin(), todo.end(), [&](JitKernel *t) { return t->src == k->src; }) == todo.end())
            todo.push_back(k);
    }
    std::vector<const std::string *> srcs;
    for (JitKernel *k : todo) srcs.push_back(&k->src);
    std::vector<std::vector<char>> code;
    std::vector<int> rcs;
    std::vector<uint8_t> hit;
    objects_parallel(srcs, code, rcs, &hit);
    for (size_t j = 0; j < todo.size(); j++) {
        int rc;
        if (rcs[j]) return rcs[j];
        hipModule_t mod;
        if (hit[j] && hipModuleLoadData(&mod, code[j].data()) != hipSuccess) {
            // a cached object the runtime refuses: a miss -- compile and replace it
            (void)hipGetLastError();
            if ((rc = rtc_compile(todo[j]->src, code[j]))) return rc;
            cache_store(todo[j]->src, code[j]);
            hit[j] = 0;
        }
        if (!hit[j] && (rc = check_hip(hipModuleLoadData(&mod, code[j].data()), "zxp jit: hipModuleLoadData")))
            return rc;
        hipFunction_t f;
        if ((rc = check_hip(hipModuleGetFunction(&f, mod, "zxp_jit"), "zxp jit: hipModuleGetFunction"))) return rc;
        c.fn.emplace(todo[j]->src, f);
    }
    for (JitKernel *k : ks) k->fn = c.fn.at(k->src);
    return 0;
}

// tables of every kernel in one buffer (zt | cp | kc | kl per kernel), one
// upload, then the launches in order on stream s
int launch_all(std::vector<JitKernel> &ks, const ZxpJitIn &in, hipStream_t s)
{
    size_t total = 0;
    for (JitKernel &K : ks) {
        K.off = total;
        K.off_cp = K.off + K.zt.size() * sizeof(JitTerm);
        K.off_kc = K.off_cp + K.cp.size() * 8;
        K.off_kl = (K.off_kc + (K.kc.size() + 1) * 8 + 15) & ~(size_t)15;  // 16-byte limb slots
        K.end = K.off_kl + (K.kl.size() + 1) * 4;
        total = (K.end + 15) & ~(size_t)15;
        K.klds = !K.split && jit_kl_lds(K.kl.size());
    }
    // The tables go through a pinned staging buffer, so the upload is
    // asynchronous and the host does not wait for the stream's earlier work
    // (a stage's kernels queued before this program): the staging buffer is
    // rewritten only after its last upload has landed (event), and the
    // device buffer after the last kernels that read it (stream order, or an
    // event if the stream changed).
    static hipEvent_t up = nullptr, use = nullptr;
    static char *pin = nullptr;
    static size_t pin_cap = 0;
    int rc;
    if (!up && ((rc = check_hip(hipEventCreateWithFlags(&up, hipEventDisableTiming), "zxp jit: event")) ||
                (rc = check_hip(hipEventCreateWithFlags(&use, hipEventDisableTiming), "zxp jit: event"))))
        return rc;
    if ((rc = check_hip(hipEventSynchronize(up), "zxp jit: staging"))) return rc;
    if (total > pin_cap) {
        if (pin) (void)hipHostFree(pin);
        pin = nullptr;
        pin_cap = 0;
        if ((rc = check_hip(hipHostMalloc((void **)&pin, total), "zxp jit: staging buffer"))) return rc;
        pin_cap = total;
    }
    char *buf = jit_buf(total, use);
    if (!buf) return set_error(ZKGPU_ERR_OOM, "zxp jit: table buffer");
    memset(pin, 0, total);
    for (JitKernel &K : ks) {
        memcpy(pin + K.off, K.zt.data(), K.zt.size() * sizeof(JitTerm));
        memcpy(pin + K.off_cp, K.cp.data(), K.cp.size() * 8);
        memcpy(pin + K.off_kc, K.kc.data(), K.kc.size() * 8);
        memcpy(pin + K.off_kl, K.kl.data(), K.kl.size() * 4);
    }
    if ((rc = check_hip(hipStreamWaitEvent(s, use, 0), "zxp jit: table order"))) return rc;
    if ((rc = check_hip(hipMemcpyAsync(buf, pin, total, hipMemcpyHostToDevice, s), "zxp jit: H2D"))) return rc;
    if ((rc = check_hip(hipEventRecord(up, s), "zxp jit: event"))) return rc;
    Ctx &c = ctx();
    const uint64_t dom = 1ULL << in.log_dom;
    for (size_t j = 0; j < ks.size(); j++) {
        JitKernel &K = ks[j];
        JitParams p;
        p.zt = (const JitTerm *)(buf + K.off);
        p.cp = (const uint64_t *const *)(buf + K.off_cp);
        p.kc = (const uint64_t *)(buf + K.off_kc);
        p.kl = (const uint32_t *)(buf + K.off_kl);
        p.xdiv = in.xdiv;
        p.xdivw = in.xdivw;
        p.zh = in.zh_dev;
        p.tw_lo = c.tw_lo[0];
        p.tw_hi = c.tw_hi[0];
        p.x_start = in.x_start;
        p.logdom = in.log_dom;
        p.logomega = in.log_omega;
        p.rmask = in.wrap ? dom - 1 : ~0ULL;
        p.zmask = in.zmask;
        p.nkl = K.klds ? (uint32_t)K.kl.size() : 0;
        p.one = 1;
        void *args[] = {&p};
        prof_begin(s);
        rc = check_hip(hipModuleLaunchKernel(K.fn, (uint32_t)((dom + JIT_THREADS - 1) / JIT_THREADS), 1, 1,
                                             JIT_THREADS, 1, 1, K.klds ? (uint32_t)(K.kl.size() * 4) : 0, s, args,
                                             nullptr),
                       "zxp jit: launch");
        char name[32];
        if (ks.size() > 1)
            snprintf(name, sizeof(name), "k_zxp_jit_s%02zu", j);  // one segment of a large program
        else
            snprintf(name, sizeof(name), "k_zxp_jit");
        prof_end(name, K.bytes, s);
        if (rc) return rc;
    }
    return check_hip(hipEventRecord(use, s), "zxp jit: event");
}

// the kernels of a program: one, or one per segment (scratch(n) returns the
// carry columns' base for n columns of ld 2^log_dom)
// An unsigned field of a code object's AMDGPU metadata note (msgpack map:
// the key string, then its value), e.g. .private_segment_fixed_size (scratch
// bytes per lane: > 0 means the kernel spills), .vgpr_count, .agpr_count.
static uint64_t co_note(const std::vector<char> &code, const char *key)
{
    const size_t kn = strlen(key);
    for (size_t at = 0; at + kn + 1 < code.size(); at++) {
        if (memcmp(code.data() + at, key, kn)) continue;
        const uint8_t *v = (const uint8_t *)code.data() + at + kn;
        const size_t left = code.size() - at - kn;
        if (v[0] < 0x80) return v[0];                                   // positive fixint
        if (v[0] == 0xcc && left > 1) return v[1];                      // uint8
        if (v[0] == 0xcd && left > 2) return ((uint64_t)v[1] << 8) | v[2];  // uint16 (big endian)
        if (v[0] == 0xce && left > 4)
            return ((uint64_t)v[1] << 24) | ((uint64_t)v[2] << 16) | ((uint64_t)v[3] << 8) | v[4];
        return 0;
    }
    return 0;
}
static uint64_t co_scratch_bytes(const std::vector<char> &code) { return co_note(code, ".private_segment_fixed_size"); }

// occupancy decisions already taken in this process: first source -> waves
// (0: keep it), so repeated evaluations do not reread code objects
static std::mutex g_waves_mu;
static std::unordered_map<std::string, uint32_t> g_waves;
static bool waves_known(const std::string &src, uint32_t &w)
{
    std::lock_guard<std::mutex> lk(g_waves_mu);
    auto it = g_waves.find(src);
    if (it == g_waves.end()) return false;
    w = it->second;
    return true;
}
static void waves_remember(const std::string &src, uint32_t w)
{
    std::lock_guard<std::mutex> lk(g_waves_mu);
    g_waves[src] = w;
}

// The same decision of a whole (unsegmented) program keyed by its structure
// -- instructions, operands, the DOT terms' sources, the launch shape; never
// the coefficient or constant values -- so that a program evaluated every
// proof is generated once per evaluation instead of twice (first source, then
// the source at the chosen occupancy; config-4 quotient).  A key shared by two
// programs can only cost one of them its occupancy target, never a result.
static uint64_t structure_key(const ZxpJitIn &in)
{
    uint64_t h = 0x9E3779B97F4A7C15ULL;
    auto mix = [&](uint64_t w) {
        h = (h ^ w) * 0xBF58476D1CE4E5B9ULL;
        h ^= h >> 31;
    };
    for (uint32_t k = 0; k < in.n_instr; k++) {
        const zxp_instr &I = in.ins[k];
        mix((uint64_t)I.op << 32 | I.dst);
        mix((uint64_t)I.a << 32 | I.b);
        if (I.op == ZXP_DOT1 || I.op == ZXP_DOT3)
            for (uint32_t t = I.a; t < I.a + I.b; t++) mix((uint64_t)in.terms[t].src << 32 | in.terms[t].comp);
    }
    for (uint32_t k = 0; k < in.n_opnd; k++) {
        const zxp_operand &o = in.opnd[k];
        mix((uint64_t)o.kind << 32 | o.a);
        mix((uint64_t)o.b << 32 | o.c);
    }
    mix((uint64_t)in.n_instr << 32 | in.n_opnd);
    mix((uint64_t)in.n_tmp1 << 32 | in.n_tmp3);
    mix((uint64_t)in.log_dom << 40 | (uint64_t)in.log_omega << 20 | in.wrap);
    mix((uint64_t)in.dot_loop_min << 32 | in.force_split);
    return h;
}
static std::unordered_map<uint64_t, uint32_t> g_waves_fp;

// may_compile = false (source / cache queries): the occupancy decisions use
// only code objects already on disk, and stop where one is missing
int build_kernels(const ZxpJitIn &in, std::vector<JitKernel> &ks, const std::function<uint64_t *(uint32_t)> &scratch,
                  int only = -1, bool may_compile = true)
{
    // code object of a source: 0 found / compiled, 1 not on disk (query mode), < 0 error
    auto object = [&](const std::string &src, std::vector<char> &code) -> int {
        if (may_compile) return code_object(src, code);
        return cache_load(src, code) ? 0 : 1;
    };
    zxp_compiled view;
    memset(&view, 0, sizeof(view));
    view.instr = in.ins;
    view.n_instr = in.n_instr;
    view.opnd = in.opnd;
    view.n_opnd = in.n_opnd;
    view.term = in.terms;
    view.n_tmp1 = in.n_tmp1;
    view.n_tmp3 = in.n_tmp3;
    const uint32_t nseg = in.n_opnd ? segments_for(view) : 1;
    int rc;
    ks.clear();
    if (nseg <= 1) {
        ks.resize(1);
        ks[0].bytes = in.bytes;
        const bool decide = in.waves_per_eu == 0 && only <= 0;
        const uint64_t fp = decide ? structure_key(in) : 0;
        if (decide) {
            uint32_t w = 0;
            bool hit;
            {
                std::lock_guard<std::mutex> lk(g_waves_mu);
                auto it = g_waves_fp.find(fp);
                hit = it != g_waves_fp.end();
                if (hit) w = it->second;
            }
            if (hit) {
                ZxpJitIn in2 = in;
                in2.waves_per_eu = w;
                return zxp_jit_build_source(in2, ks[0]);
            }
        }
        if ((rc = zxp_jit_build_source(in, ks[0]))) return rc;
        // A kernel the compiler leaves at 169-256 registers runs 2 waves per
        // SIMD and is latency-bound: compiled again with an occupancy target
        // of 3 (<= 168; config-4 quotient 186 VGPRs, 15.3 -> 12.7 ms); one
        // above 256 (1 wave, AGPRs: the reference's step2prev, 512 + spills)
        // with a target of 2.  Kernels at 3+ waves are left alone (a target
        // lets the scheduler spend registers: FRI polynomial 8.9 -> 9.2 ms),
        // as are block-split programs (registers bounded by their blocks).
        // Decided from the code object's metadata, so the prebuilt cache and
        // the run agree.
        if (decide) {
            uint32_t w = 0;
            if (!ks[0].split && !waves_known(ks[0].src, w)) {
                std::vector<char> code;
                if ((rc = object(ks[0].src, code))) return rc < 0 ? rc : 0;  // (query mode: undecided)
                const uint64_t regs = co_note(code, ".vgpr_count") + co_note(code, ".agpr_count");
                w = regs > 256 ? 2 : regs > 168 ? 3 : 0;
                waves_remember(ks[0].src, w);
            }
            {
                std::lock_guard<std::mutex> lk(g_waves_mu);
                g_waves_fp[fp] = w;
            }
            if (w) {
                ZxpJitIn in2 = in;
                in2.waves_per_eu = w;
                if ((rc = zxp_jit_build_source(in2, ks[0]))) return rc;
            }
        }
        return 0;
    }
    std::vector<ZxpSegment> seg;
    uint32_t n_scratch = 0;
    if ((rc = zxp_segment(view, nseg, seg, n_scratch))) return rc;
    uint64_t *scr = scratch(std::max<uint32_t>(1, n_scratch));
    if (!scr) return ZKGPU_ERR_OOM;
    const uint64_t dom = 1ULL << in.log_dom;
    ks.resize(seg.size());
    // The segments are independent: their sources are generated (and their
    // occupancy decided) in parallel threads -- on the zkEVM-shaped quotient
    // ~10 ms of host work per segment, 8 segments, each proof (the GPU waits
    // for it).  The occupancy memo and the disk cache are thread-safe.
    auto one = [&](size_t j) -> int {
        int rc;
        ZxpJitIn J = in;
        J.ins = seg[j].instr.data();
        J.n_instr = (uint32_t)seg[j].instr.size();
        J.opnd = seg[j].opnd.data();
        J.n_opnd = (uint32_t)seg[j].opnd.size();
        J.terms = seg[j].term.data();
        J.force_split = 1;
        // occupancy target of a segment (seg_waves): 4 waves per SIMD (128
        // VGPRs; the 512-byte blocks keep fewer values live than the round-5
        // 1024-byte ones, which spilled up to 348 bytes with the prefetch).
        // A segment whose code spills more than spill_max bytes per lane
        // (300) at that target is compiled again one wave
        // lower (down to 2): the reference's step3 segments spill 324-452
        // bytes at 4 waves, none at 2.
        const uint32_t seg_waves = seg_ab().waves ? seg_ab().waves : 4;
        constexpr uint64_t spill_max = 300;
        const bool fixed = J.waves_per_eu != 0;
        J.scratch = scr;
        J.scratch_ld = dom;
        uint32_t w = fixed ? J.waves_per_eu : seg_waves;
        J.waves_per_eu = w;
        if ((rc = zxp_jit_build_source(J, ks[j]))) return rc;  // 1: unsupported shape -> interpreter for the whole program
        if (!fixed && (only < 0 || (size_t)only == j)) {
            const std::string first = ks[j].src;
            uint32_t wk = 0;
            if (waves_known(first, wk)) {
                if (wk != w) {
                    J.waves_per_eu = wk;
                    if ((rc = zxp_jit_build_source(J, ks[j]))) return rc;
                }
            } else {
                bool known = true;
                while (w > 2) {
                    std::vector<char> code;
                    if ((rc = object(ks[j].src, code)) < 0) return rc;
                    if (rc) {  // query mode, not compiled yet: undecided
                        known = false;
                        break;
                    }
                    if (co_scratch_bytes(code) <= spill_max) break;
                    J.waves_per_eu = --w;
                    if ((rc = zxp_jit_build_source(J, ks[j]))) return rc;
                }
                if (known) waves_remember(first, w);
            }
        }
        ks[j].bytes = in.bytes / seg.size() + 8.0 * (seg[j].carry_in + seg[j].carry_out) * (double)dom;
        return 0;
    };
    std::vector<int> rcs(seg.size(), 0);
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t j; (j = next++) < seg.size();) rcs[j] = one(j);
    };
    std::vector<std::thread> th;
    const size_t nthr = std::min<size_t>(seg.size(), std::max(1u, std::min(8u, std::thread::hardware_concurrency())));
    for (size_t t = 1; t < nthr; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
    for (int r : rcs)
        if (r) return r;  // the first failing segment in order (1: unsupported shape -> the interpreter)
    return 0;
}

}  // namespace

int zxp_jit_run(const ZxpJitIn &in, hipStream_t s)
{
    std::vector<JitKernel> ks;
    int rc = build_kernels(in, ks, [&](uint32_t n) { return workspace(6, (size_t)n << in.log_dom << 3); });
    if (rc) return rc;
    std::vector<JitKernel *> pk;
    for (JitKernel &K : ks) pk.push_back(&K);
    if ((rc = compile_all(pk))) return rc;
    return launch_all(ks, in, s);
}

}  // namespace zk

// Diagnostics (C-ABI, include/zkgpu.h): compile a program as
// zkgpu_zxp_eval_dev would and print its straight-line kernel source;
// optionally run hiprtc on it.  No GPU needed.
extern "C" int zkgpu_zxp_jit_source(const void *instr, uint32_t n_instr, const void *opnd, uint32_t n_opnd,
                                    uint32_t n_tmp1, uint32_t n_tmp3, const uint64_t *challenges,
                                    const uint64_t *publics, uint32_t n_publics, const uint64_t *evals,
                                    uint32_t n_evals, char *buf, uint64_t buflen, int rtc_check)
{
    using namespace zk;
    zxp_compiled cp;
    int rc = zkgpu_zxp_compile(instr, n_instr, opnd, n_opnd, n_tmp1, n_tmp3, challenges, publics, n_publics, evals,
                               n_evals, 0, &cp);
    if (rc) return rc;
    // placeholder sections: pointers are kernel inputs, not part of the source
    static uint64_t dummy;
    zkgpu_sections S;
    for (int k = 0; k < 12; k++) {
        S.sec[k] = &dummy;
        S.ld[k] = 1;
        S.ncols[k] = 0;
    }
    const ZxpJitIn J = zxp_jit_in(cp, &S, challenges, publics, evals);  // as zkgpu_zxp_eval_dev (api.hip)
    std::vector<JitKernel> ks;
    static uint64_t dummy_scratch;
    const char *only_env = getenv("ZKGPU_ZXP_JIT_ONLY");
    if ((rc = build_kernels(J, ks, [](uint32_t) { return &dummy_scratch; }, only_env ? atoi(only_env) : -1,
                            rtc_check == 1 || rtc_check == 2)))
        return rc < 0 ? rc : set_error(ZKGPU_ERR_ARG, "zxp jit: unsupported program shape");
    std::string src;  // the kernels' sources (one per segment)
    for (size_t j = 0; j < ks.size(); j++) {
        if (ks.size() > 1) src += "// ---- segment " + std::to_string(j) + " of " + std::to_string(ks.size()) + "\n";
        src += ks[j].src;
    }
    if (buf && buflen) {
        const size_t n = std::min<size_t>(src.size(), buflen - 1);
        memcpy(buf, src.data(), n);
        buf[n] = 0;
    }
    if (rtc_check == 3) {  // cache query only: 1 = every compiled object on disk
        std::vector<char> code;
        for (const JitKernel &K : ks)
            if (!cache_load(K.src, code)) return 0;
        return 1;
    }
    if (rtc_check) {
        // compile (or find in the disk cache); rtc_check == 2 also writes the
        // code objects to $ZKGPU_ZXP_JIT_DUMP (.<segment> appended when there
        // are several; register / scratch inspection)
        // ZKGPU_ZXP_JIT_ONLY=j: only segment j (tools/jit_prebuild.py runs the
        // segments in parallel processes: hiprtc serialises threads)
        std::vector<const std::string *> srcs;
        std::vector<size_t> idx;
        for (size_t j = 0; j < ks.size(); j++)
            if (!only_env || (size_t)atoi(only_env) == j) {
                srcs.push_back(&ks[j].src);
                idx.push_back(j);
            }
        std::vector<std::vector<char>> code;
        std::vector<int> rcs;
        objects_parallel(srcs, code, rcs);
        for (int r : rcs)
            if (r) return r;
        const char *dump = getenv("ZKGPU_ZXP_JIT_DUMP");
        if (rtc_check == 2 && dump)
            for (size_t j = 0; j < code.size(); j++) {
                const std::string path = ks.size() > 1 ? std::string(dump) + "." + std::to_string(idx[j]) : dump;
                FILE *f = fopen(path.c_str(), "wb");
                if (f) {
                    fwrite(code[j].data(), 1, code[j].size(), f);
                    fclose(f);
                }
            }
    }
    return (int)std::min<size_t>(src.size(), 0x7FFFFFFF);
}
