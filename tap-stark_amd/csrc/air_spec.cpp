// hiprtc's time grows faster than the program (a 4.6k-instruction program compiles in 14 s, an
// 18.8k one in 146 s: profiles/r06_air_jit_compile.txt), so the specialisation has a budget:
//   <= TS_JIT_SYNC_INSTR (default 2048, ~3 s)   compiled inside ts_air_compile, as before;
//   <= TS_JIT_MAX_INSTR  (default 32768)        compiled by a child process (ts_jitc): proofs run on the
//                                               interpreter (a GPU path too) until the code object is
//                                               ready, the next use loads it; ts_air_jit_wait joins;
//   larger                                      interpreter only.
// The segmented form (ts_air_compile_opts, air.cpp plan_segments) compiles linearly and has no such budget:
// always in the background, its kernels split into up to J modules, one child each.
// Both kernels compute the same words, so which one ran never shows in a proof.
// A background compilation runs in a CHILD PROCESS (tap-stark_amd/jitc/ts_jitc.cpp, built beside the
// library): hiprtc serialises compilations inside one process, cannot be interrupted, and a thread still
// inside it when the host exits meets the compiler's static destructors.  The child compiles beside the
// prover and beside other children, is killed when its AIR is freed, and leaves nothing behind but a
// code object in a private temporary directory.  Every route ends in publish().
#include "air_spec.hpp"

#include <dlfcn.h>
#include <errno.h>
#include <signal.h>
#include <spawn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <thread>

#include "jit.hpp"

extern char** environ;

namespace ts {

namespace {

std::string jitc_path() {
    if (const char* e = getenv("TS_JITC_PATH")) return e;
    Dl_info info;
    if (dladdr((void*)&jitc_path, &info) && info.dli_fname) {
        std::string p = info.dli_fname;
        const size_t k = p.rfind('/');
        return (k == std::string::npos ? std::string(".") : p.substr(0, k)) + "/ts_jitc";
    }
    return "ts_jitc";
}

size_t env_or(const char* name, size_t dflt) {
    const char* v = getenv(name);
    return v && *v ? (size_t)strtoull(v, nullptr, 10) : dflt;
}

// One compiler child per module.  `pid` stays set until the child has been reaped (or is known to have
// ended when the host reaped it first), so a live child is always killed with its AIR.
struct JitChild {
    pid_t pid = -1;
    bool done = false, ok = false;
    std::string src, out, log, cache;
    std::vector<char> code;  // the code object, once done and ok
};
bool file_exists(const std::string& f) { return !f.empty() && access(f.c_str(), F_OK) == 0; }
// waitpid without losing the child to EINTR; ECHILD (the host ignores SIGCHLD or reaped it with
// waitpid(-1)) counts as ended only once ts_jitc's last file is there (it writes the log after the code
// object, both by rename) or the pid is gone.  true once the child has ended; `st` is valid if `reaped`.
bool child_ended(JitChild& c, bool wait, bool& reaped, int& st) {
    reaped = false;
    for (;;) {
        const pid_t r = waitpid(c.pid, &st, wait ? 0 : WNOHANG);
        if (r == c.pid) {
            reaped = true;
            return true;
        }
        if (r == 0) return false;
        if (errno == EINTR) continue;
        if (file_exists(c.log) || file_exists(c.out) || (kill(c.pid, 0) != 0 && errno == ESRCH)) return true;
        if (!wait) return false;
        std::this_thread::sleep_for(std::chrono::milliseconds(20));
    }
}
pid_t spawn(const std::string& helper, const std::string& arch, const JitChild& c) {
    char* argv[] = {const_cast<char*>(helper.c_str()), const_cast<char*>(arch.c_str()),
                    const_cast<char*>(c.src.c_str()), const_cast<char*>(c.out.c_str()),
                    const_cast<char*>(c.log.c_str()), nullptr};
    // the child is a plain compiler run: nothing preloaded into the host (profilers, sanitizer runtimes)
    // belongs in it
    std::vector<char*> envp;
    for (char** e = environ; e && *e; e++)
        if (strncmp(*e, "LD_PRELOAD=", 11) != 0 && strncmp(*e, "HSA_TOOLS_LIB=", 14) != 0 &&
            strncmp(*e, "ROCP_TOOL_", 10) != 0)
            envp.push_back(*e);
    envp.push_back(nullptr);
    pid_t pid = -1;
    return posix_spawn(&pid, helper.c_str(), nullptr, nullptr, argv, envp.data()) == 0 ? pid : -1;
}

// the calling thread on `device` for this scope (device < 0: wherever it is); the caller's device is restored
struct OnDevice {
    int prev = -1;
    explicit OnDevice(int device) {
        if (device >= 0) (void)hipGetDevice(&prev);
        if (device >= 0 && prev != device) (void)hipSetDevice(device);
        else prev = -1;
    }
    ~OnDevice() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace

struct JitJob {
    std::string dir;
    std::vector<JitChild> mods;
    std::chrono::steady_clock::time_point t0;
    ~JitJob() {
        for (JitChild& c : mods) {
            if (c.pid > 0) {  // still compiling for an AIR nobody wants any more
                (void)kill(c.pid, SIGKILL);
                int st = 0;
                while (waitpid(c.pid, &st, 0) < 0 && errno == EINTR) {
                }
            }
            for (const std::string& f : {c.src, c.out, c.out + ".part", c.log, c.log + ".part"})
                if (!f.empty() && !dir.empty()) (void)unlink(f.c_str());
        }
        if (!dir.empty()) (void)rmdir(dir.c_str());
    }
};

// The modules of one AIR, loaded on its device, and the kernel set made of them: the one owner of a loaded
// module, whether the set was published or abandoned half-loaded.
struct LoadedKernels {
    JitKernelSet set;
    const int device;
    explicit LoadedKernels(int dev) : device(dev) {}
    ~LoadedKernels() {
        OnDevice here(device);
        for (void* m : set.modules) (void)hipModuleUnload((hipModule_t)m);
    }
};

SpecialisedAir::SpecialisedAir(Context* ctx, const uint32_t* tape, size_t n_words, uint32_t segment_instr,
                               uint32_t jit_jobs) {
    prog_ = compile_air(tape, n_words);
    const size_t n_instr = prog_.code.size() / 4;
    // segmented: the plan (host only).  The register budget keeps every segment kernel within 128 VGPRs
    // (4 waves per SIMD) with no spill; TS_SEG_REGS overrides it for measurements.
    if (segment_instr != 0 && n_instr > segment_instr) {
        seg_ = std::make_unique<SegmentPlan>(plan_segments(prog_, segment_instr, (uint32_t)env_or("TS_SEG_REGS", 32)));
        jit_jobs_ = std::min<uint32_t>(jit_jobs ? jit_jobs : 4, (uint32_t)seg_->segs.size());
    }
    if (!ctx) return;  // host-only AIR (no GPU needed): usable by ts_verify
    device_ = ctx->device;
    code_ = DevBuf<uint32_t>(ctx, std::max<size_t>(prog_.code.size(), 4));
    if (!prog_.code.empty())
        TS_HIP(hipMemcpyAsync(code_.p, prog_.code.data(), prog_.code.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    ctx->sync();
    prog_.d_code = code_.p;
    // specialise the quotient kernel for this AIR (the interpreter runs it otherwise)
    arch_ = ctx->arch_name;
    if (getenv("TS_NO_JIT")) {
        log_ = "disabled by TS_NO_JIT";
    } else if (seg_) {
        start_background();  // always in the background: J children, or the cache
    } else if (n_instr <= env_or("TS_JIT_SYNC_INSTR", 2048)) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<char> code;
        if (!jit_compile_source(source(), arch_.c_str(), code, log_) || !publish({code})) state_ = JIT_FAILED;
        seconds_ = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } else if (n_instr <= env_or("TS_JIT_MAX_INSTR", 32768)) {
        start_background();  // one child, or the cache
    } else {
        log_ = "program above TS_JIT_MAX_INSTR: interpreter only";
    }
}

SpecialisedAir::~SpecialisedAir() = default;

std::string SpecialisedAir::source() const {
    return seg_ ? jit_segment_sources(prog_, *seg_, 1)[0] : jit_quotient_source(prog_);
}
std::vector<std::string> SpecialisedAir::module_kernels(uint32_t j, uint32_t n_modules) const {
    if (!seg_) return {"k_quotient_jit"};
    std::vector<std::string> names;
    for (uint32_t k = jit_segment_module_first(*seg_, n_modules, j); k < jit_segment_module_first(*seg_, n_modules, j + 1);
         k++)
        names.push_back("k_quotient_seg" + std::to_string(k));
    return names;
}

// loads every module on the AIR's device (the caller's device is restored) and publishes the set whole
bool SpecialisedAir::publish(const std::vector<std::vector<char>>& codes) {
    auto ks = std::make_unique<LoadedKernels>(device_);
    ks->set.seg = seg_.get();
    {
        OnDevice here(device_);
        for (uint32_t j = 0; j < codes.size(); j++)
            if (!jit_load_module(codes[j], module_kernels(j, (uint32_t)codes.size()), ks->set, log_)) return false;
    }
    kernels_ = std::move(ks);
    prog_.jit.publish(&kernels_->set);
    state_ = JIT_LOADED;
    return true;
}

// one child per module that the cache does not hold; with every module cached the set is published at once
void SpecialisedAir::start_background() {
    const std::vector<std::string> srcs =
        seg_ ? jit_segment_sources(prog_, *seg_, jit_jobs_) : std::vector<std::string>{source()};
    auto j = std::make_unique<JitJob>();
    j->t0 = std::chrono::steady_clock::now();
    j->mods.resize(srcs.size());
    bool need_child = false;
    for (size_t m = 0; m < srcs.size(); m++) {
        JitChild& c = j->mods[m];
        c.cache = jit_cache_path(srcs[m], arch_.c_str());
        if (jit_cache_load(c.cache, c.code)) c.done = c.ok = true;
        else need_child = true;
    }
    if (!need_child) {  // code objects of these very sources left by an earlier process: a job that has ended
        job_ = std::move(j);
        return poll(false);
    }
    const std::string helper = jitc_path();
    if (access(helper.c_str(), X_OK) != 0) {
        log_ = "background specialisation needs the helper " + helper + " (not found): interpreter only";
        return;
    }
    const char* tmp = getenv("TMPDIR");
    std::string tmpl = std::string(tmp && *tmp ? tmp : "/tmp") + "/ts_jit_XXXXXX";
    std::vector<char> buf(tmpl.begin(), tmpl.end());
    buf.push_back(0);
    if (!mkdtemp(buf.data())) {
        log_ = "mkdtemp failed: interpreter only";
        return;
    }
    j->dir = buf.data();
    for (size_t m = 0; m < srcs.size(); m++) {
        JitChild& c = j->mods[m];
        if (c.done) continue;
        const std::string stem = j->dir + (seg_ ? "/quotient_seg" + std::to_string(m) : std::string("/quotient_jit"));
        c.src = stem + ".hip";
        c.out = stem + ".co";
        c.log = seg_ ? stem + ".log" : j->dir + "/log.txt";
        FILE* f = fopen(c.src.c_str(), "wb");
        if (!f || fwrite(srcs[m].data(), 1, srcs[m].size(), f) != srcs[m].size()) {
            if (f) fclose(f);
            log_ = "cannot write the kernel source: interpreter only";
            return;  // ~JitJob kills the children already started
        }
        fclose(f);
        c.pid = spawn(helper, arch_, c);
        if (c.pid <= 0) {
            c.pid = -1;
            log_ = "posix_spawn of " + helper + " failed: interpreter only";
            return;
        }
    }
    job_ = std::move(j);
    state_ = JIT_COMPILING;
}

// called on the thread that drives the context: once every module has ended, publish the set or fail
void SpecialisedAir::poll(bool wait) {
    std::lock_guard<std::mutex> pg(poll_m_);
    if (!job_) return;
    for (JitChild& c : job_->mods) {
        if (c.done) continue;
        bool reaped = false;
        int st = 0;
        if (!child_ended(c, wait, reaped, st)) return;  // still compiling
        c.pid = -1;
        c.done = true;
        c.ok = (!reaped || (WIFEXITED(st) && WEXITSTATUS(st) == 0)) && read_file(c.out, c.code) && !c.code.empty();
        if (c.ok) jit_cache_store(c.cache, c.code);
    }
    seconds_ = std::chrono::duration<double>(std::chrono::steady_clock::now() - job_->t0).count();
    std::vector<std::vector<char>> codes;
    bool ok = true;
    for (JitChild& c : job_->mods) {
        if (!c.ok && ok) {
            std::vector<char> l;
            if (read_file(c.log, l)) log_.assign(l.data(), std::min<size_t>(l.size(), 4096));
            if (log_.empty()) log_ = "the compiler child ended without a code object";
        }
        ok = ok && c.ok;
        codes.push_back(std::move(c.code));
    }
    if (!ok || !publish(codes)) state_ = JIT_FAILED;
    job_.reset();
}

}  // namespace ts
