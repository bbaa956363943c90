// ab_batch_sample.cpp -- InferenceEngine::generate_batch of n default-config (sampled) requests on the
// host-sampler loop (TI_BATCH_SAMPLE_DEVICE=0: a device step, n x vocab logits to the host and a sort per request,
// every step) against the device route (ti_engine_generate_sampled with n streams); DESIGN 4.9.  The output is
// kept in profiles/sampled_loops_ab.txt.
//
//   ab_batch_sample [n = 8] [prompt_len = 8] [max_new = 128] [rounds = 3]
//
// The seeded synthetic INT4 Llama-2-7B shape (a tensorless ModelData with turboinfer.synthetic = 1), default
// InferenceConfig but for max_sequence_length and max_batch_size.  The two routes alternate A B A B in this one
// process (the knob is read per call), one untimed call of each first; wall clock of the call, new tokens per
// second over all requests (a request may stop early at EOS: the tokens actually returned are counted).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <vector>

#include "turboinfer/turboinfer.hpp"

using namespace turboinfer;

int main(int argc, char** argv) {
  try {
    const int n = argc > 1 ? std::atoi(argv[1]) : 8, plen = argc > 2 ? std::atoi(argv[2]) : 8;
    const int max_new = argc > 3 ? std::atoi(argv[3]) : 128, rounds = argc > 4 ? std::atoi(argv[4]) : 3;
    model::ModelData md;
    auto& m = md.metadata();
    m.name = "ab_batch_sample";
    m.architecture = "llama";
    m.vocab_size = 32000;
    m.hidden_size = 4096;
    m.num_layers = 32;
    m.num_heads = 32;
    m.intermediate_size = 11008;
    m.rope_theta = 10000.0f;
    m.extra_params["turboinfer.synthetic"] = "1";
    model::InferenceConfig cfg;   // top_k 50, top_p 0.9, temperature 1.0
    cfg.max_sequence_length = (size_t)(plen + max_new + 8);
    cfg.max_batch_size = (size_t)n;
    model::InferenceEngine eng(md, cfg);
    std::vector<std::vector<int>> prompts(n);
    for (int i = 0; i < n; ++i)
      for (int t = 0; t < plen; ++t) prompts[i].push_back(3 + (int)((1103515245u * (unsigned)(i * plen + t + 1) + 12345u) % 31000u));
    std::printf("generate_batch: synthetic INT4 llama2-7b, %d default-config requests, %d-token prompts, %d new tokens, "
                "%d alternating rounds\n", n, plen, max_new, rounds);
    std::vector<double> tps[2];
    for (int r = 0; r <= rounds; ++r)      // round 0 untimed (graph capture)
      for (int dev = 0; dev < 2; ++dev) {
        setenv("TI_BATCH_SAMPLE_DEVICE", dev ? "1" : "0", 1);
        const auto t0 = std::chrono::steady_clock::now();
        const auto res = eng.generate_batch(prompts, (size_t)max_new, false);
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        size_t gen = 0;
        for (size_t i = 0; i < res.size(); ++i) gen += res[i].tokens.size() - prompts[i].size();
        if (r) tps[dev].push_back((double)gen / s);
        std::printf("  round %d %-11s %6zu tokens in %8.1f ms  %8.1f tok/s%s\n", r, dev ? "device" : "host loop", gen, s * 1e3,
                    (double)gen / s, r ? "" : "  (untimed)");
        std::fflush(stdout);
      }
    for (int dev = 0; dev < 2; ++dev) {
      std::sort(tps[dev].begin(), tps[dev].end());
      std::printf("  %-11s median %8.1f tok/s [%8.1f .. %8.1f]\n", dev ? "device" : "host loop", tps[dev][tps[dev].size() / 2],
                  tps[dev].front(), tps[dev].back());
    }
    return 0;
  } catch (const std::exception& e) {
    std::cerr << "ab_batch_sample: " << e.what() << "\n";
    return 2;
  }
}
