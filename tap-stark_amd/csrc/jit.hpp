// hiprtc specialisation of the quotient kernel (jit.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "air.hpp"

namespace ts {

// HIP source of the specialised kernel (exposed for tests / inspection)
std::string jit_quotient_source(const AirProgram& air);
// segmented form: the kernels k_quotient_seg<k> of plan.segs split into n_modules sources (contiguous runs
// of segments; module j holds segments [seg_first(j), seg_first(j + 1)))
std::vector<std::string> jit_segment_sources(const AirProgram& air, const SegmentPlan& plan, uint32_t n_modules);
uint32_t jit_segment_module_first(const SegmentPlan& plan, uint32_t n_modules, uint32_t j);
// the gfx code object of that source (hiprtc; needs no GPU): false with the reason / compiler output in `log`
bool jit_compile_source(const std::string& src, const char* arch, std::vector<char>& code, std::string& log);
bool read_file(const std::string& path, std::vector<char>& out);
// TS_JIT_CACHE_DIR: "" when unset; load checks the ELF magic; store writes beside and renames
std::string jit_cache_path(const std::string& src, const char* arch);
bool jit_cache_load(const std::string& path, std::vector<char>& code);
void jit_cache_store(const std::string& path, const std::vector<char>& code);
// loads a code object on the current device and resolves the named kernels, appending the module and the
// functions (in the order of `names`) to `set`.  On false (reason appended to `log`) `set` may hold the module
// already: whoever owns the set unloads it either way.
bool jit_load_module(const std::vector<char>& code, const std::vector<std::string>& names, JitKernelSet& set,
                     std::string& log);

}  // namespace ts
