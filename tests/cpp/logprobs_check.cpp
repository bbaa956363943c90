// logprobs_check.cpp -- drives InferenceEngine::compute_logprobs for tests/test_cpp_logprobs.py.
//
//   logprobs_check <model_dir> <tokens> <weight_bits> <out>
//
// model_dir/manifest.txt: "meta vocab hidden layers heads inter rope_theta" then "<name> <file>"
// lines, and arrays as small binary files, both as tests/cpp/api_check.cpp reads them:
//   u32 dtype (0 f32, 1 i32, 2 i8) | u32 ndim | u64 dims[ndim] | raw little-endian data
// tokens: i32 [n]; out: f32 [n], element i = log p(tokens[i]) under the logits of position i.
// An exception (empty or out-of-vocabulary input, a device error) is printed and exits with 2.
#include <cstdint>
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

static void write_floats(const std::string& path, const std::vector<float>& v) {
  std::ofstream f(path, std::ios::binary);
  const uint32_t head[2] = {0, 1};
  const uint64_t n = v.size();
  f.write((const char*)head, 8);
  f.write((const char*)&n, 8);
  if (n) f.write((const char*)v.data(), (std::streamsize)(n * sizeof(float)));
}

int main(int argc, char** argv) {
  try {
    if (argc != 5) throw std::runtime_error("usage: logprobs_check <model_dir> <tokens> <weight_bits> <out>");
    const std::string dir = argv[1];
    model::ModelData md;
    std::ifstream man(dir + "/manifest.txt");
    std::string tag;
    man >> tag >> md.metadata().vocab_size >> md.metadata().hidden_size >> md.metadata().num_layers >>
        md.metadata().num_heads >> md.metadata().intermediate_size >> md.metadata().rope_theta;
    if (tag != "meta") throw std::runtime_error("manifest: expected meta line");
    md.metadata().name = "logprobs_check";
    md.metadata().architecture = "llama";
    std::string name, file;
    while (man >> name >> file) md.add_tensor(name, read_array(dir + "/" + file));
    md.metadata().extra_params["turboinfer.weight_bits"] = argv[3];   // (the MI355X option)
    const Tensor tt = read_array(argv[2]);
    const size_t n = tt.shape().total_size();
    std::vector<int> tokens;
    if (n) tokens.assign(tt.data_ptr<int32_t>(), tt.data_ptr<int32_t>() + n);
    model::InferenceConfig cfg;
    cfg.max_sequence_length = 64;
    model::InferenceEngine eng(md, cfg);
    const std::vector<float> lp = eng.compute_logprobs(tokens);
    if (lp.size() != tokens.size()) throw std::runtime_error("compute_logprobs: wrong result length");
    write_floats(argv[4], lp);
    return 0;
  } catch (const std::exception& e) {
    std::cerr << "logprobs_check: " << e.what() << "\n";
    return 2;
  }
}
