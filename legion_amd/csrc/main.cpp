// main.cpp -- the `sampling_server` binary.  Reference: sampling_server/src/main.cu:5-16
// (argv = <gpu_number> <cache_agg_mode>, fan-out hard-coded {25,10}).  This build accepts the
// fan-out as optional extra arguments (the reference's pybind Run(fanout, ...) signature,
// sampling_server/sampling_server.cpp:7): sampling_server <gpu_number> <cache_agg_mode> [f1 f2 ...] [--disk] [--feature-dtype bf16]
// --disk = Run()'s in_memory_mode 0: meta_config carries fifteen fields and the caches are the hybrid CPU-cache / GPU-cache tier
// --feature-dtype bf16: the feature table and every cache tier hold bfloat16 rows (legion_hip.h LEGION_FEATURE_BF16); the
// trainer still receives float32 rows.  --feature-dtype f32 is the default.
// --feature-out-dtype bf16: the trainer receives bfloat16 rows (legion_server_set_feature_out_dtype), whatever the storage dtype;
// --feature-out-dtype f32 is the default.
// --sample-replace 0: every pool samples without replacement (legion_server_set_sample_replace); 1, the reference's draw with
// replacement, is the default.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/legion_hip.h"

int main(int argc, char** argv)
{
    if (argc < 3) {
        std::printf("usage: %s <gpu_number> <cache_agg_mode> [fanout ...] [--disk] [--feature-dtype f32|bf16] [--feature-out-dtype f32|bf16] [--sample-replace 0|1]\n", argv[0]);
        return 2;
    }
    std::vector<int32_t> fanout;
    int32_t in_memory_mode = 1;
    for (int i = 3; i < argc; i++) {
        if (std::strcmp(argv[i], "--disk") == 0) in_memory_mode = 0;
        else if (std::strcmp(argv[i], "--feature-dtype") == 0) {
            const char* v = i + 1 < argc ? argv[++i] : "";
            const int32_t dtype = std::strcmp(v, "bf16") == 0 ? LEGION_FEATURE_BF16 : std::strcmp(v, "f32") == 0 ? LEGION_FEATURE_F32 : -1;
            if (legion_server_set_feature_dtype(dtype) != 0) {
                std::printf("--feature-dtype: expected f32 or bf16, got '%s'\n", v);
                return 2;
            }
        } else if (std::strcmp(argv[i], "--feature-out-dtype") == 0) {
            const char* v = i + 1 < argc ? argv[++i] : "";
            const int32_t dtype = std::strcmp(v, "bf16") == 0 ? LEGION_FEATURE_BF16 : std::strcmp(v, "f32") == 0 ? LEGION_FEATURE_F32 : -1;
            if (legion_server_set_feature_out_dtype(dtype) != 0) {
                std::printf("--feature-out-dtype: expected f32 or bf16, got '%s'\n", v);
                return 2;
            }
        } else if (std::strcmp(argv[i], "--sample-replace") == 0) {
            const char* v = i + 1 < argc ? argv[++i] : "";
            const int32_t replace = std::strcmp(v, "1") == 0 ? 1 : std::strcmp(v, "0") == 0 ? 0 : -1;
            if (legion_server_set_sample_replace(replace) != 0) {
                std::printf("--sample-replace: expected 0 or 1, got '%s'\n", v);
                return 2;
            }
        } else fanout.push_back(std::atoi(argv[i]));
    }
    if (fanout.empty()) { fanout.push_back(25); fanout.push_back(10); }
    return legion_run(fanout.data(), (int32_t)fanout.size(), std::atoi(argv[1]), in_memory_mode, (int)std::atof(argv[2]));
}
