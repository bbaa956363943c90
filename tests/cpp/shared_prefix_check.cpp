// shared_prefix_check.cpp -- drives InferenceEngine::generate_batch with requests that share a prompt prefix, for
// tests/test_cpp_shared_prefix.py.
//
//   shared_prefix_check <model_dir> <weight_bits> <prompts> <max_new>
//
// model_dir/manifest.txt and the array files: as tests/cpp/logprobs_check.cpp reads them.
// prompts: i32 [n][len], one request per row, padded with -1 behind each request's last token.
// Environment (read by the library): TI_SHARE_PREFIX, TI_SHARE_MIN, TI_KV_BITS.
// Runs, each from reset_state(): "greedy" (top_k 1), "again" (the same call once more: a registered prefix is found
// registered) and "logprobs" (top_k 1 with include_logprobs: the sampled device loop).  Prints, per run,
// "run <name> req <i> tokens ..." (the new tokens) and "run <name> forward_passes <n>" (the "Forward Passes" line
// of performance_stats()).  An exception is printed and exits with 2.
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "turboinfer/turboinfer.hpp"

using namespace turboinfer;
using core::DataType;
using core::Tensor;
using core::TensorShape;

static Tensor read_array(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error("cannot open " + path);
  uint32_t code = 0, nd = 0;
  f.read((char*)&code, 4);
  f.read((char*)&nd, 4);
  std::vector<size_t> dims(nd);
  for (auto& d : dims) {
    uint64_t v = 0;
    f.read((char*)&v, 8);
    d = (size_t)v;
  }
  const DataType dt = code == 0 ? DataType::kFloat32 : code == 1 ? DataType::kInt32 : DataType::kInt8;
  Tensor t(TensorShape(dims), dt);
  if (t.byte_size()) f.read((char*)t.data(), (std::streamsize)t.byte_size());
  if (!f) throw std::runtime_error("short read " + path);
  return t;
}

static long forward_passes(const model::InferenceEngine& eng) {
  std::istringstream is(eng.performance_stats());
  std::string line;
  const std::string key = "Forward Passes:";
  while (std::getline(is, line)) {
    const size_t at = line.find(key);
    if (at != std::string::npos) return std::atol(line.c_str() + at + key.size());
  }
  throw std::runtime_error("performance_stats() has no Forward Passes line");
}

static void run(model::InferenceEngine& eng, const std::string& name, const std::vector<std::vector<int>>& prompts,
                size_t max_new, bool logprobs) {
  eng.reset_state();
  const auto res = eng.generate_batch(prompts, max_new, logprobs);
  if (res.size() != prompts.size()) throw std::runtime_error("generate_batch: result count");
  for (size_t i = 0; i < res.size(); ++i) {
    const auto& r = res[i];
    if (r.tokens.size() < prompts[i].size()) throw std::runtime_error("generate_batch: tokens shorter than the prompt");
    for (size_t t = 0; t < prompts[i].size(); ++t)
      if (r.tokens[t] != prompts[i][t]) throw std::runtime_error("generate_batch: the result does not start with the prompt");
    std::cout << "run " << name << " req " << i << " tokens";
    for (size_t t = prompts[i].size(); t < r.tokens.size(); ++t) std::cout << " " << r.tokens[t];
    std::cout << "\n";
  }
  std::cout << "run " << name << " forward_passes " << forward_passes(eng) << "\n";
}

int main(int argc, char** argv) {
  try {
    if (argc != 5) throw std::runtime_error("usage: shared_prefix_check <model_dir> <weight_bits> <prompts> <max_new>");
    const std::string dir = argv[1];
    model::ModelData md;
    std::ifstream man(dir + "/manifest.txt");
    std::string tag;
    man >> tag >> md.metadata().vocab_size >> md.metadata().hidden_size >> md.metadata().num_layers >>
        md.metadata().num_heads >> md.metadata().intermediate_size >> md.metadata().rope_theta;
    if (tag != "meta") throw std::runtime_error("manifest: expected meta line");
    md.metadata().name = "shared_prefix_check";
    md.metadata().architecture = "llama";
    std::string name, file;
    while (man >> name >> file) md.add_tensor(name, read_array(dir + "/" + file));
    md.metadata().extra_params["turboinfer.weight_bits"] = argv[2];   // (the MI355X options)
    const Tensor tt = read_array(argv[3]);
    if (tt.shape().ndim() != 2) throw std::runtime_error("prompts: expected [n][len]");
    const size_t n = tt.shape().size(0), len = tt.shape().size(1);
    std::vector<std::vector<int>> prompts(n);
    for (size_t i = 0; i < n; ++i)
      for (size_t t = 0; t < len && tt.data_ptr<int32_t>()[i * len + t] >= 0; ++t)
        prompts[i].push_back(tt.data_ptr<int32_t>()[i * len + t]);
    const size_t max_new = (size_t)std::atoi(argv[4]);
    model::InferenceConfig cfg;
    cfg.max_sequence_length = 64;
    cfg.max_batch_size = 4;
    cfg.top_k = 1;
    model::InferenceEngine eng(md, cfg);
    run(eng, "greedy", prompts, max_new, false);
    run(eng, "again", prompts, max_new, false);
    run(eng, "logprobs", prompts, max_new, true);
    return 0;
  } catch (const std::exception& e) {
    std::cerr << "shared_prefix_check: " << e.what() << "\n";
    return 2;
  }
}
