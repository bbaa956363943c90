// lookahead_check.cpp -- drives InferenceEngine::generate with the lookahead option for tests/test_cpp_lookahead.py.
//
//   lookahead_check <model_dir> <prompt> <weight_bits> <lookahead> <max_new> <out>
//
// model_dir/manifest.txt and the array files: as tests/cpp/logprobs_check.cpp reads them.
// lookahead: the value of extra_params["turboinfer.lookahead"], or "-" to leave the option absent.
// prompt: i32 [n]; out: i32 [prompt + new tokens] as generate() returns them (top_k = 1: greedy).
// An exception (a bad option value, a device error) is printed and exits with 2.
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

static void write_ints(const std::string& path, const std::vector<int>& v) {
  std::ofstream f(path, std::ios::binary);
  const uint32_t head[2] = {1, 1};
  const uint64_t n = v.size();
  f.write((const char*)head, 8);
  f.write((const char*)&n, 8);
  for (int x : v) {
    const int32_t y = x;
    f.write((const char*)&y, 4);
  }
}

int main(int argc, char** argv) {
  try {
    if (argc != 7) throw std::runtime_error("usage: lookahead_check <model_dir> <prompt> <weight_bits> <lookahead|-> <max_new> <out>");
    const std::string dir = argv[1];
    model::ModelData md;
    std::ifstream man(dir + "/manifest.txt");
    std::string tag;
    man >> tag >> md.metadata().vocab_size >> md.metadata().hidden_size >> md.metadata().num_layers >>
        md.metadata().num_heads >> md.metadata().intermediate_size >> md.metadata().rope_theta;
    if (tag != "meta") throw std::runtime_error("manifest: expected meta line");
    md.metadata().name = "lookahead_check";
    md.metadata().architecture = "llama";
    std::string name, file;
    while (man >> name >> file) md.add_tensor(name, read_array(dir + "/" + file));
    md.metadata().extra_params["turboinfer.weight_bits"] = argv[3];   // (the MI355X options)
    if (std::string(argv[4]) != "-") md.metadata().extra_params["turboinfer.lookahead"] = argv[4];
    const Tensor tt = read_array(argv[2]);
    const size_t n = tt.shape().total_size();
    std::vector<int> prompt(tt.data_ptr<int32_t>(), tt.data_ptr<int32_t>() + n);
    model::InferenceConfig cfg;
    cfg.max_sequence_length = 64;
    cfg.top_k = 1;
    model::InferenceEngine eng(md, cfg);
    const model::GenerationResult r = eng.generate(prompt, (size_t)std::atoi(argv[5]));
    write_ints(argv[6], r.tokens);
    std::cout << "stop_reason " << r.stop_reason << " finished " << r.finished << "\n";
    return 0;
  } catch (const std::exception& e) {
    std::cerr << "lookahead_check: " << e.what() << "\n";
    return 2;
  }
}
