// guide_check.cpp -- drives InferenceEngine::generate / generate_batch / generate_beam_search under the guide_file
// option (token-automaton guided decoding), for tests/test_cpp_guide.py.
//
//   guide_check <model_dir> <weight_bits> <prompts> <max_new> <top_k> [key=value ...]
//
// model_dir/manifest.txt and the array files: as tests/cpp/logprobs_check.cpp reads them.
// prompts: i32 [n][len], one request per row, padded with -1 behind each request's last token.
// key=value: entries of extra_params (turboinfer.guide_file, turboinfer.lookahead, ...).
// Environment (read by the library): TI_GUIDE_FILE, TI_BATCH_SAMPLE_DEVICE, TI_LOOKAHEAD.
// Runs with top_k as given (1: a greedy config), temperature 0.8, top_p 0.9, each from reset_state(): "batch"
// (generate_batch of every request), "alone" (generate of request 0) and "logprobs" (generate_batch with
// include_logprobs).  Prints "run <name> req <i> tokens ..." (the new tokens), then "beam ok" or "beam threw
// <message>" for a generate_beam_search of request 0; when it threw, the message goes to stderr too and the exit
// status is 3.  An exception anywhere else is printed and exits with 2.
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <iostream>
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

static void print(const std::string& name, size_t i, const std::vector<int>& prompt, const model::GenerationResult& r) {
  if (r.tokens.size() < prompt.size()) throw std::runtime_error("tokens shorter than the prompt");
  for (size_t t = 0; t < prompt.size(); ++t)
    if (r.tokens[t] != prompt[t]) throw std::runtime_error("the result does not start with the prompt");
  std::cout << "run " << name << " req " << i << " tokens";
  for (size_t t = prompt.size(); t < r.tokens.size(); ++t) std::cout << " " << r.tokens[t];
  std::cout << "\n";
}

int main(int argc, char** argv) {
  try {
    if (argc < 6) throw std::runtime_error("usage: guide_check <model_dir> <weight_bits> <prompts> <max_new> <top_k> [key=value ...]");
    const std::string dir = argv[1];
    model::ModelData md;
    std::ifstream man(dir + "/manifest.txt");
    std::string tag;
    man >> tag >> md.metadata().vocab_size >> md.metadata().hidden_size >> md.metadata().num_layers >>
        md.metadata().num_heads >> md.metadata().intermediate_size >> md.metadata().rope_theta;
    if (tag != "meta") throw std::runtime_error("manifest: expected meta line");
    md.metadata().name = "guide_check";
    md.metadata().architecture = "llama";
    std::string name, file;
    while (man >> name >> file) md.add_tensor(name, read_array(dir + "/" + file));
    md.metadata().extra_params["turboinfer.weight_bits"] = argv[2];   // (the MI355X options)
    for (int i = 6; i < argc; ++i) {
      const std::string kv = argv[i];
      const size_t eq = kv.find('=');
      if (eq == std::string::npos) throw std::runtime_error("expected key=value, got " + kv);
      md.metadata().extra_params[kv.substr(0, eq)] = kv.substr(eq + 1);
    }
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
    cfg.top_k = (size_t)std::atoi(argv[5]);
    cfg.temperature = 0.8f;
    cfg.top_p = 0.9f;
    model::InferenceEngine eng(md, cfg);
    eng.reset_state();
    auto res = eng.generate_batch(prompts, max_new, false);
    for (size_t i = 0; i < res.size(); ++i) print("batch", i, prompts[i], res[i]);
    eng.reset_state();
    print("alone", 0, prompts[0], eng.generate(prompts[0], max_new, false));
    eng.reset_state();
    res = eng.generate_batch(prompts, max_new, true);
    for (size_t i = 0; i < res.size(); ++i) print("logprobs", i, prompts[i], res[i]);
    eng.reset_state();
    try {
      eng.generate_beam_search(prompts[0], 2, 2, false);
      std::cout << "beam ok\n";
    } catch (const std::runtime_error& e) {
      std::cout << "beam threw " << e.what() << "\n";
      std::cerr << "guide_check: beam search: " << e.what() << "\n";
      return 3;
    }
    return 0;
  } catch (const std::exception& e) {
    std::cerr << "guide_check: " << e.what() << "\n";
    return 2;
  }
}
