// One AIR as the provers use it (air_spec.cpp): the lowered program, its device copy, the optional
// segment plan, and the lifecycle of its hiprtc specialisation -- which route compiles it, the compiler
// children of the background route, the loaded modules and the published kernel set.
#pragma once
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "air.hpp"
#include "context.hpp"

namespace ts {

struct JitJob;
struct LoadedKernels;

class SpecialisedAir {
public:
    // what ts_air_jit_wait reports (the numbers are ABI)
    enum State { JIT_NONE = 0, JIT_COMPILING = 1, JIT_LOADED = 3, JIT_FAILED = 4 };

    // ctx == nullptr: a host-only AIR (degree rules, the verifier): no GPU, never specialised.
    // segment_instr == 0: the monolithic route; S > 0 and a program longer than S: the segmented one, its
    // kernels in up to jit_jobs modules (0: 4).  Throws ts::Error on a malformed tape.
    SpecialisedAir(Context* ctx, const uint32_t* tape, size_t n_words, uint32_t segment_instr, uint32_t jit_jobs);
    ~SpecialisedAir();  // kills and reaps children still compiling, removes their files, unloads the modules

    // the program as the prover sees it, with a background specialisation adopted if it has finished.  Called
    // on the thread that drives the context, once per proof: with no job pending it is one lock and one
    // pointer test.
    const AirProgram& ready() {
        poll(false);
        return prog_;
    }
    // blocks until a background specialisation has ended: the state, and the seconds the compilation took
    std::pair<State, double> wait() {
        poll(true);
        return {state_, seconds_};
    }
    bool is_specialised() { return ready().jit.load() != nullptr; }
    const AirProgram& prog() const { return prog_; }
    const Context* context() const { return code_.ctx; }  // the context it was compiled on; null: host-only
    const SegmentPlan* seg() const { return seg_.get(); }
    std::string source() const;  // the HIP source of the whole specialisation, as one module

private:
    std::vector<std::string> module_kernels(uint32_t j, uint32_t n_modules) const;
    bool publish(const std::vector<std::vector<char>>& codes);
    void start_background();
    void poll(bool wait);

    AirProgram prog_;
    DevBuf<uint32_t> code_;
    std::unique_ptr<SegmentPlan> seg_;  // set: the segmented form
    uint32_t jit_jobs_ = 1;             // modules (= compiler children) of the segmented form
    int device_ = -1;                   // the device the modules are loaded on (-1: host-only AIR)
    std::string arch_;
    State state_ = JIT_NONE;
    double seconds_ = 0;
    std::string log_;  // why there is no specialisation (a debugging aid: read in a debugger, no ABI call returns it)
    std::mutex poll_m_;  // two threads proving with one AIR: the adoption happens once
    std::unique_ptr<JitJob> job_;
    std::unique_ptr<LoadedKernels> kernels_;  // what prog_.jit points at once published
};

}  // namespace ts
