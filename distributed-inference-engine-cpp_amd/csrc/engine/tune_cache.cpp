#include "tune_cache.h"

#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <sstream>

namespace die {

std::string tune_cache_path(const EngineOptions& opt) {
  std::string p = opt.tune_cache;
  if (p == "auto") {  // (the Python layer resolves $DIE_TUNE_CACHE before it gets here)
    if (const char* h = std::getenv("HOME")) p = std::string(h) + "/.cache/die_amd/tune.json";
    else p.clear();
  }
  return p;
}

size_t load_tune_cache(const std::string& path, const std::string& arch_name, TuneMap& out) {
  if (path.empty()) return 0;
  std::ifstream f(path);
  if (!f) return 0;
  try {
    std::stringstream ss;
    ss << f.rdbuf();
    const Json j = Json::parse(ss.str());
    const Json* arch = j.find(arch_name);
    if (!arch) return 0;
    for (const auto& kv : arch->as_object()) {
      const auto& a = kv.second.as_array();
      if (a.size() < 4) continue;
      out[kv.first] = {Tune{static_cast<int>(a[0].as_int()), static_cast<int>(a[1].as_int()), a[2].as_bool(),
                            a.size() > 4 ? static_cast<int>(a[4].as_int()) : 0,
                            a.size() > 5 ? static_cast<int>(a[5].as_int()) : 0,
                            a.size() > 6 ? static_cast<int>(a[6].as_int()) : 0},
                       a[3].as_double()};
    }
  } catch (const std::exception&) {
    return 0;  // unreadable cache: retune
  }
  return out.size();
}

void save_tune_cache(const std::string& path, const std::string& arch_name, const TuneMap& shapes) {
  if (path.empty()) return;
  try {
    Json root = Json::object();
    {
      std::ifstream f(path);
      if (f) {
        std::stringstream ss;
        ss << f.rdbuf();
        root = Json::parse(ss.str());
      }
    }
    Json arch = root.find(arch_name) ? *root.find(arch_name) : Json::object();
    for (const auto& kv : shapes) {
      Json a = Json::array();
      a.push_back(kv.second.first.tile);
      a.push_back(kv.second.first.splits);
      a.push_back(kv.second.first.fused);
      a.push_back(kv.second.second);
      a.push_back(kv.second.first.order);
      a.push_back(kv.second.first.tail);
      a.push_back(kv.second.first.sk);
      arch[kv.first] = a;
    }
    root[arch_name] = arch;
    const auto slash = path.rfind('/');
    if (slash != std::string::npos) {  // no shell: this process owns a GPU context
      std::error_code ec;
      std::filesystem::create_directories(path.substr(0, slash), ec);
    }
    const std::string tmp = path + ".tmp" + std::to_string(getpid());
    {
      std::ofstream o(tmp);
      o << root.dump();
    }
    std::rename(tmp.c_str(), path.c_str());
  } catch (const std::exception&) {
  }
}

}  // namespace die
