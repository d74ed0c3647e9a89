// The opaque handle types of include/tapstark.h, shared by the translation units that implement
// the C ABI (abi.cpp, taptree.cpp, comm.cpp).  Each wraps the ts:: object that does the work; an AIR's is
// ts::SpecialisedAir (air_spec.hpp).
#pragma once
#include <memory>

#include "../../include/tapstark.h"
#include "air_spec.hpp"
#include "host.hpp"
#include "logup.hpp"

struct ts_ctx {
    ts::Context ctx;
    explicit ts_ctx(int dev) : ctx(dev) {}
};
struct ts_air {
    ts::SpecialisedAir a;
};
struct ts_matrix {
    ts::DeviceMatrix m;
};
struct ts_pcs_data {
    std::unique_ptr<ts::PcsData> d;
};
// the key of a multi-table proof: the committed batch and, with keep_values, the row-major inputs as handles the
// caller may borrow (ts_multi_key_values)
struct ts_multi_key {
    ts::MultiKey k;
    std::vector<std::unique_ptr<ts_matrix>> values;
};
