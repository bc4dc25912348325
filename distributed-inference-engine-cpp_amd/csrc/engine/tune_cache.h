// Autotune persistence (kernel configs cached in a tuning file): one JSON object per
// GPU architecture, shape key -> [tile, splits, fused, us, order, tail, sk].
#pragma once

#include <map>
#include <string>
#include <utility>

#include "engine.h"

namespace die {

struct Tune {
  int tile = 0;
  int splits = 1;
  bool fused = false;  // split-K reduced in-kernel by the last split block (else a second kernel)
  int order = 0;       // ConvArgs::order (0 heuristic, 1 N-fastest, 2 M-fastest)
  int tail = 0;        // ConvArgs::tail (> 0: split-K on the last partial round's tiles only)
  int sk = 0;          // ConvArgs::sk (> 0: stream-K launch of sk blocks; splits/tail unused)
};

// shape key -> (winner, its time in us)
using TuneMap = std::map<std::string, std::pair<Tune, double>>;

// EngineOptions::tune_cache resolved to a file name ("" = no cache)
std::string tune_cache_path(const EngineOptions& opt);
// Adds the file's entries for `arch` to `out`; returns out.size(), or 0 when there is nothing usable.
size_t load_tune_cache(const std::string& path, const std::string& arch, TuneMap& out);
// Merges `shapes` into the file's entries for `arch` (written to a temporary, then renamed).
void save_tune_cache(const std::string& path, const std::string& arch, const TuneMap& shapes);

}  // namespace die
