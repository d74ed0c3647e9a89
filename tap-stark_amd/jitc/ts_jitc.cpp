// ts_jitc -- out-of-process hiprtc compilation for libtapstark_hip.so's background specialisation of
// large AIRs (csrc/air_spec.cpp).  hiprtc serialises compilations inside one process and cannot be
// interrupted; a child process compiles beside the prover (and beside other children), can be killed
// when its AIR is freed, and takes the compiler's global state with it when it ends.  It never touches
// the GPU (hiprtc only).
//
//     ts_jitc <arch> <source.hip> <out.co> <log.txt>        exit 0 = code object written
//
// The log is written last, on every path (empty if the compiler said nothing), and like the code object by
// rename: a parent that could not reap the child (ECHILD) takes the log's presence for "ended".
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

typedef void* rtcProgram;

static bool read_file(const char* path, std::string& out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
    fclose(f);
    return true;
}
static void write_file(const char* path, const void* p, size_t n) {
    // write beside, then rename: the reader never sees a partial file
    const std::string tmp = std::string(path) + ".part";
    if (FILE* f = fopen(tmp.c_str(), "wb")) {
        fwrite(p, 1, n, f);
        fclose(f);
        (void)rename(tmp.c_str(), path);
    }
}

int main(int argc, char** argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: ts_jitc <arch> <source.hip> <out.co> <log.txt>\n");
        return 2;
    }
    const char *arch = argv[1], *src_path = argv[2], *out_path = argv[3], *log_path = argv[4];
    std::string src;
    if (!read_file(src_path, src)) {
        write_file(log_path, "cannot read the source", 22);
        return 1;
    }
    void* lib = nullptr;
    for (const char* name : {"libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"})
        if ((lib = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
    if (!lib) {
        write_file(log_path, "libhiprtc not available", 23);
        return 1;
    }
    auto create = (int (*)(rtcProgram*, const char*, const char*, int, const char**, const char**))dlsym(lib, "hiprtcCreateProgram");
    auto compile = (int (*)(rtcProgram, int, const char**))dlsym(lib, "hiprtcCompileProgram");
    auto log_size = (int (*)(rtcProgram, size_t*))dlsym(lib, "hiprtcGetProgramLogSize");
    auto get_log = (int (*)(rtcProgram, char*))dlsym(lib, "hiprtcGetProgramLog");
    auto code_size = (int (*)(rtcProgram, size_t*))dlsym(lib, "hiprtcGetCodeSize");
    auto get_code = (int (*)(rtcProgram, char*))dlsym(lib, "hiprtcGetCode");
    if (!create || !compile || !log_size || !get_log || !code_size || !get_code) {
        write_file(log_path, "libhiprtc lacks an entry point", 30);
        return 1;
    }
    rtcProgram prog = nullptr;
    if (create(&prog, src.c_str(), "quotient_jit.hip", 0, nullptr, nullptr) != 0) {
        write_file(log_path, "hiprtcCreateProgram failed", 26);
        return 1;
    }
    const std::string arch_opt = std::string("--offload-arch=") + arch;
    const char* opts[] = {arch_opt.c_str(), "-O3"};
    const int rc = compile(prog, 2, opts);
    size_t sz = 0;
    log_size(prog, &sz);
    std::vector<char> log(sz > 1 ? sz : 1);
    if (sz > 1) get_log(prog, log.data());
    const size_t log_n = sz > 1 ? sz - 1 : 0;
    if (rc != 0) {
        write_file(log_path, log.data(), log_n);
        return 1;
    }
    code_size(prog, &sz);
    std::vector<char> code(sz);
    get_code(prog, code.data());
    write_file(out_path, code.data(), sz);
    write_file(log_path, log.data(), log_n);
    return 0;
    // (no hiprtcDestroyProgram / dlclose: the process ends here)
}
