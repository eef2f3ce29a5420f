// Stand-alone check of the plan cache (csrc/plan.cpp) under concurrent opens, meant for ThreadSanitizer.  Host only, no GPU:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=thread -ffp-contract=off -o plan_cache_race tools/plan_cache_race.cpp \
//       foo_dsp_resampler_amd/csrc/plan.cpp foo_dsp_resampler_amd/csrc/design.cpp -lpthread && ./plan_cache_race
//
// Eight threads look up four configs over and over, as the plugin's converter threads do when they open (chain.h:36); one of them
// clears the cache now and then, so that hits, misses, insertions of the same key by two threads and evictions all happen beside
// each other.  Every plan handed out is compared, bit for bit, with the one design_plan gives on the main thread.  Exit status 0 and
// "ok" when every lookup matched (a data race is ThreadSanitizer's to report: it makes the exit status non-zero by itself).
#include "../foo_dsp_resampler_amd/csrc/plan.hpp"

#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

namespace {

bool same_bits(const std::vector<double> &a, const std::vector<double> &b)
{
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}

bool same_plan(const rsmp::ChainPlan &a, const rsmp::ChainPlan &b)
{
  return a.describe() == b.describe() && a.isamp_max == b.isamp_max && same_bits(a.poly_table, b.poly_table) &&
         same_bits(a.dft[0].taps, b.dft[0].taps) && same_bits(a.dft[1].taps, b.dft[1].taps);
}

} // namespace

int main()
{
  std::vector<rsmp::Config> cfgs(4);
  cfgs[0].in_rate = 44100, cfgs[0].out_rate = 48000;
  cfgs[1].in_rate = 44100, cfgs[1].out_rate = 96000;
  cfgs[2].in_rate = 96000, cfgs[2].out_rate = 44100;
  cfgs[3].in_rate = 44100, cfgs[3].out_rate = 48000, cfgs[3].phase = 25; // (not linear phase: the slow design)
  std::vector<rsmp::ChainPlan> want(cfgs.size());
  for (size_t i = 0; i < cfgs.size(); ++i)
    if (rsmp::design_plan(cfgs[i], want[i]) != 0) {
      std::fprintf(stderr, "config %zu refused\n", i);
      return 2;
    }
  rsmp::Config refused = cfgs[0];
  refused.phase = 101;

  const int kThreads = 8, kRounds = 200;
  std::atomic<long> wrong{0}, lookups{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < kThreads; ++t)
    pool.emplace_back([&, t] {
      for (int r = 0; r < kRounds; ++r) {
        const size_t i = size_t(t + r) % cfgs.size();
        rsmp::ChainPlan got;
        if (rsmp::make_plan(cfgs[i], got) != 0 || !same_plan(got, want[i])) ++wrong;
        ++lookups;
        if (r % 16 == 5 && rsmp::make_plan(refused, got) == 0) ++wrong; // a refusal beside the others: never kept
        if (t == 0 && r % 64 == 63) rsmp::plan_cache_clear();
        if (t == 1 && r % 8 == 0) {
          int entries = 0;
          rsmp::plan_cache_stats(nullptr, nullptr, &entries);
          if (entries < 0 || entries > rsmp::kPlanCacheMax) ++wrong;
        }
      }
    });
  for (std::thread &th : pool) th.join();
  unsigned long long hits = 0, misses = 0;
  int entries = 0;
  rsmp::plan_cache_stats(&hits, &misses, &entries);
  std::printf("%ld lookups on %d threads, %ld wrong; since the last clear: %llu hits, %llu misses, %d entries\n", lookups.load(), kThreads,
              wrong.load(), hits, misses, entries);
  if (wrong.load() || entries > int(cfgs.size())) return 1;
  std::printf("ok\n");
  return 0;
}
