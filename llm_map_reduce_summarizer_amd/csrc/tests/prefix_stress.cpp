// Multi-threaded stress of the KV page allocator's prefix index (csrc/runtime/page_alloc.cpp), built and
// run under AddressSanitizer + UndefinedBehaviorSanitizer and, separately, ThreadSanitizer by
// tests/test_prefix_sanitizers.py.  Host code only.
//
//   T threads play sequences against one allocator: match a prompt, allocate the pages the match did not
//   bring, "write" the new prompt pages (a shadow table of what every page holds), publish the full prompt
//   pages, hold them for a while, release.  The prompts come from a few families that share heads of
//   different lengths, and the pool is small, so matches, duplicate publishes and evictions all race.
//   Checked all along: a matched page holds exactly the tokens of its position in the chain (so no page was
//   recycled while findable); a page that alloc hands out has no holder (no page is free and referenced);
//   the shadow holder counts stay >= 0.  At the end: every reference is back (holders 0, available ==
//   total - reserved, free + evictable), a double release and a foreign id are refused, and reset leaves an
//   empty index with the same count available.
// Exit status 0 = pass; the sanitizers abort with a report on any memory error or data race.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

extern "C" {
void* mrsum_pages_create(int num_pages, int reserved);
int mrsum_pages_alloc(void* h, int n, int* out);
int mrsum_pages_free(void* h, int n, const int* ids);
int mrsum_pages_available(void* h);
void mrsum_pages_destroy(void* h);
int mrsum_pages_match(void* h, const int* toks, int n_toks, int* out);
int mrsum_pages_publish(void* h, const int* toks, int n_toks, const int* pages, int n_full);
int mrsum_pages_release(void* h, int n, const int* ids);
void mrsum_pages_reset(void* h);
int mrsum_pages_cached(void* h);
long long mrsum_pages_evictions(void* h);
}

#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

namespace {

constexpr int P = 64;

// prompt `variant` of `family`: the first `shared` pages are the family's, the rest the variant's own
std::vector<int> make_prompt(int family, int variant, int shared, int n_toks) {
  std::vector<int> t(n_toks);
  for (int i = 0; i < n_toks; ++i) {
    const int page = i / P;
    const int who = page < shared ? family * 1000 : family * 1000 + 1 + variant;
    t[i] = (who * 131 + page * 17 + (i % P) * 3) % 100000;
  }
  return t;
}

// what a page at position `page` of prompt `t` holds: a hash of the prompt up to the page's end
uint64_t chain_tag(const std::vector<int>& t, int page) {
  uint64_t h = 1469598103934665603ull;
  for (int i = 0; i < (page + 1) * P; ++i) h = (h ^ static_cast<uint32_t>(t[i])) * 1099511628211ull;
  return h | 1;
}

struct Held {
  std::vector<int> pages;
};

}  // namespace

int main() {
  const int total = 96, reserved = 1, threads = 8, iters = 3000;
  void* h = mrsum_pages_create(total, reserved);
  CHECK(h != nullptr);
  std::vector<std::atomic<int>> holders(total);
  std::vector<std::atomic<uint64_t>> content(total);
  for (auto& x : holders) x.store(0);
  for (auto& x : content) x.store(0);
  std::atomic<long long> hits{0}, published{0};
  std::vector<std::thread> ts;
  for (int t = 0; t < threads; ++t) {
    ts.emplace_back([&, t] {
      std::mt19937 rng(99 + t);
      std::vector<Held> held;
      auto drop = [&](size_t k) {
        std::vector<int> pages = std::move(held[k].pages);
        held.erase(held.begin() + static_cast<long>(k));
        for (int id : pages) CHECK(holders[id].fetch_sub(1) >= 1);
        CHECK(mrsum_pages_release(h, static_cast<int>(pages.size()), pages.data()) == 0);
      };
      for (int it = 0; it < iters; ++it) {
        if (!held.empty() && (held.size() >= 3 || rng() % 3 == 0)) {
          drop(rng() % held.size());
          continue;
        }
        const int family = static_cast<int>(rng() % 8), variant = static_cast<int>(rng() % 6);
        const int shared = 1 + family % 3;
        const int n_toks = 1 + static_cast<int>(rng() % (6 * P));
        const std::vector<int> toks = make_prompt(family, variant, shared, n_toks);
        const int need = (n_toks + 1 + P - 1) / P;  // the prompt and one generated token
        std::vector<int> pages(static_cast<size_t>(need) + 8);
        const int m = mrsum_pages_match(h, toks.data(), n_toks, pages.data());
        CHECK(m >= 0 && m <= (n_toks - 1) / P && m <= need);
        for (int i = 0; i < m; ++i) {
          const int id = pages[i];
          CHECK(id >= reserved && id < total);
          holders[id].fetch_add(1);
          CHECK(content[id].load() == chain_tag(toks, i));  // the page of exactly these tokens
        }
        hits += m;
        if (mrsum_pages_alloc(h, need - m, pages.data() + m) != 0) {
          for (int i = 0; i < m; ++i) CHECK(holders[pages[i]].fetch_sub(1) >= 1);
          CHECK(mrsum_pages_release(h, m, pages.data()) == 0);
          continue;
        }
        pages.resize(need);
        for (int i = m; i < need; ++i) {
          const int id = pages[i];
          CHECK(id >= reserved && id < total);
          CHECK(holders[id].fetch_add(1) == 0);  // nobody held what alloc handed out
          content[id].store((i + 1) * P <= n_toks ? chain_tag(toks, i) : 0);
        }
        const int n_full = n_toks / P;
        const int added = mrsum_pages_publish(h, toks.data(), n_toks, pages.data(), n_full);
        CHECK(added >= 0 && added <= n_full - m);
        published += added;
        held.push_back(Held{std::move(pages)});
      }
      while (!held.empty()) drop(held.size() - 1);
    });
  }
  for (auto& th : ts) th.join();
  for (auto& x : holders) CHECK(x.load() == 0);
  CHECK(mrsum_pages_available(h) == total - reserved);
  CHECK(hits.load() > 0 && published.load() > 0 && mrsum_pages_evictions(h) > 0);
  CHECK(mrsum_pages_cached(h) > 0 && mrsum_pages_cached(h) <= total - reserved);
  // single-threaded: refusals, and a published page survives its holder
  const std::vector<int> toks = make_prompt(9, 0, 1, 2 * P + 5);
  int pg[3], again[3];
  CHECK(mrsum_pages_alloc(h, 3, pg) == 0);
  CHECK(mrsum_pages_publish(h, toks.data(), 2 * P + 5, pg, 2) == 2);
  CHECK(mrsum_pages_publish(h, toks.data(), 2 * P + 5, pg, 3) == -1);  // page 3 is not full
  CHECK(mrsum_pages_release(h, 3, pg) == 0);
  CHECK(mrsum_pages_release(h, 1, pg) == -1);  // double release refused
  const int foreign[2] = {0, total + 5};
  CHECK(mrsum_pages_release(h, 1, &foreign[0]) == -1);
  CHECK(mrsum_pages_release(h, 1, &foreign[1]) == -1);
  CHECK(mrsum_pages_match(h, toks.data(), 2 * P + 5, again) == 2 && again[0] == pg[0] && again[1] == pg[1]);
  CHECK(mrsum_pages_match(h, toks.data(), 2 * P, again) == 1);  // one token at least is left to compute
  const int both[3] = {pg[0], pg[1], pg[0]};
  CHECK(mrsum_pages_release(h, 3, both) == -1);  // a page named twice in one call: nothing released
  CHECK(mrsum_pages_release(h, 2, both) == 0);
  CHECK(mrsum_pages_release(h, 1, pg) == 0);
  CHECK(mrsum_pages_available(h) == total - reserved);
  mrsum_pages_reset(h);
  CHECK(mrsum_pages_cached(h) == 0);
  CHECK(mrsum_pages_available(h) == total - reserved);
  CHECK(mrsum_pages_match(h, toks.data(), 2 * P + 5, again) == 0);
  mrsum_pages_destroy(h);
  std::printf("prefix stress ok\n");
  return 0;
}
