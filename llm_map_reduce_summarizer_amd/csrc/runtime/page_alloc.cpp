// KV-cache page allocator (host C++), used by engine/kv_cache.py.
//
// LIFO free list over page ids [reserved, num_pages): recently freed pages
// are reused first (they are the most likely to still sit in the 256 MiB
// Infinity Cache / L2).  An allocation is all-or-nothing.  A per-page
// reference count catches double frees and foreign ids.  Thread-safe.
//
// Prefix index (KV prefix caching): a page that holds 64 prompt tokens can be
// PUBLISHED as a node of a chain -- (parent node, its 64 token ids) -- and is
// then found again by MATCHing a prompt that begins with the same tokens.  A
// node is named by its page id (a page is at most one node; -1 = the root).
// The lookup hashes (parent, ids) and then compares the ids themselves, so a
// hash collision can never produce a hit.  A page may have several holders
// (reference count); a published page nobody holds keeps its content and stays
// findable ("evictable") until alloc runs out of free pages and takes the least
// recently used evictable page, dropping the nodes below it with it (their
// pages go back to the free list once nobody holds them): no reachable node
// ever has a missing ancestor.  A chain is marked used leaf first, so its head
// is its most recent page and a chain is eaten from its tail.  With the index
// never used every call returns what the plain free list returned.
//
// C ABI (ctypes):
//   void* mrsum_pages_create(int num_pages, int reserved)
//   int   mrsum_pages_alloc(void*, int n, int* out)      0 ok, -1 not enough pages
//   int   mrsum_pages_free(void*, int n, const int* ids) 0 ok, -1 bad / double free (nothing freed)
//   int   mrsum_pages_available(void*)                   free + evictable pages
//   void  mrsum_pages_destroy(void*)
//   int   mrsum_pages_match(void*, const int* toks, int n_toks, int* out)
//           longest cached chain of full pages that prefixes toks, at most (n_toks - 1) / 64 pages;
//           takes a reference on each; returns their number
//   int   mrsum_pages_publish(void*, const int* toks, int n_toks, const int* pages, int n_full)
//           registers the caller's first n_full pages (held by it) as the chain of toks; where a node
//           exists already it stays and the caller's page stays private; returns the nodes added, -1 bad
//   int   mrsum_pages_release(void*, int n, const int* ids)   == mrsum_pages_free: drops one reference each
//   void  mrsum_pages_reset(void*)                       forgets every node (held pages stay allocated)
//   int   mrsum_pages_cached(void*)                      nodes in the index
//   long long mrsum_pages_evictions(void*)               nodes dropped by alloc so far

#include <cstdint>
#include <cstring>
#include <mutex>
#include <set>
#include <unordered_map>
#include <utility>
#include <vector>

namespace {

constexpr int PAGE_TOKENS = 64;

struct Pages {
  std::vector<int> free_list;
  std::vector<int> refs;            // holders of a page; reserved pages: 1 forever
  std::vector<uint8_t> cached;      // the page is a node of the index
  std::vector<int> parent;          // node: page id of its parent node, -1 = root
  std::vector<std::vector<int>> kids;
  std::vector<uint64_t> tick;       // last use (match / publish) of a node
  std::vector<int32_t> toks;        // node: its 64 token ids
  std::unordered_multimap<uint64_t, int> by_hash;
  std::set<std::pair<uint64_t, int>> evictable;  // (tick, page): cached pages nobody holds
  uint64_t clock = 0;
  long long evictions = 0;
  int n_cached = 0;
  int reserved = 0;
  std::mutex mu;
};

uint64_t node_hash(int parent, const int32_t* t) {
  uint64_t h = 1469598103934665603ull ^ static_cast<uint32_t>(parent);
  for (int i = 0; i < PAGE_TOKENS; ++i) {
    h *= 1099511628211ull;
    h ^= static_cast<uint32_t>(t[i]);
  }
  return h * 1099511628211ull;
}

// the node (parent, t), or -1
int find_node(Pages* p, int parent, const int32_t* t) {
  auto range = p->by_hash.equal_range(node_hash(parent, t));
  for (auto it = range.first; it != range.second; ++it) {
    const int id = it->second;
    if (p->parent[id] == parent &&
        std::memcmp(&p->toks[static_cast<size_t>(id) * PAGE_TOKENS], t, PAGE_TOKENS * sizeof(int32_t)) == 0)
      return id;
  }
  return -1;
}

// forget node `id`; `unlink`: take it off its parent's list (not needed when the parent goes too).  A page
// nobody holds returns to the free list
void drop_node(Pages* p, int id, bool unlink) {
  const int32_t* t = &p->toks[static_cast<size_t>(id) * PAGE_TOKENS];
  const int par = p->parent[id];
  auto range = p->by_hash.equal_range(node_hash(par, t));
  for (auto it = range.first; it != range.second; ++it)
    if (it->second == id) {
      p->by_hash.erase(it);
      break;
    }
  if (unlink && par >= 0) {
    auto& k = p->kids[par];
    for (size_t i = 0; i < k.size(); ++i)
      if (k[i] == id) {
        k.erase(k.begin() + static_cast<long>(i));
        break;
      }
  }
  p->cached[id] = 0;
  p->parent[id] = -1;
  --p->n_cached;
  if (p->refs[id] == 0) {
    p->evictable.erase({p->tick[id], id});
    p->free_list.push_back(id);
  }
}

// forget `root` and every node below it; returns the nodes dropped
int drop_subtree(Pages* p, int root) {
  std::vector<int> stack{root};
  int n = 0;
  while (!stack.empty()) {
    const int id = stack.back();
    stack.pop_back();
    for (int c : p->kids[id]) stack.push_back(c);
    p->kids[id].clear();
    drop_node(p, id, id == root);
    ++n;
  }
  return n;
}

void touch(Pages* p, int id) {
  if (p->refs[id] == 0) p->evictable.erase({p->tick[id], id});
  p->tick[id] = ++p->clock;
  if (p->refs[id] == 0) p->evictable.insert({p->tick[id], id});
}

int release_locked(Pages* p, int n, const int* ids) {
  const int total = static_cast<int>(p->refs.size());
  for (int i = 0; i < n; ++i) {
    const int id = ids[i];
    if (id < p->reserved || id >= total || p->refs[id] <= 0) return -1;
    for (int j = 0; j < i; ++j)
      if (ids[j] == id) return -1;
  }
  for (int i = n - 1; i >= 0; --i) {
    const int id = ids[i];
    if (--p->refs[id] > 0) continue;
    if (p->cached[id])
      p->evictable.insert({p->tick[id], id});
    else
      p->free_list.push_back(id);
  }
  return 0;
}

}  // namespace

extern "C" {

void* mrsum_pages_create(int num_pages, int reserved) {
  if (num_pages <= reserved || reserved < 0) return nullptr;
  auto* p = new Pages();
  p->reserved = reserved;
  p->refs.assign(num_pages, 0);
  for (int i = 0; i < reserved; ++i) p->refs[i] = 1;
  p->cached.assign(num_pages, 0);
  p->parent.assign(num_pages, -1);
  p->kids.resize(num_pages);
  p->tick.assign(num_pages, 0);
  p->free_list.reserve(num_pages - reserved);
  for (int i = num_pages - 1; i >= reserved; --i) p->free_list.push_back(i);
  return p;
}

int mrsum_pages_alloc(void* h, int n, int* out) {
  auto* p = static_cast<Pages*>(h);
  std::lock_guard<std::mutex> g(p->mu);
  if (n < 0 || static_cast<size_t>(n) > p->free_list.size() + p->evictable.size()) return -1;
  for (int i = 0; i < n; ++i) {
    if (p->free_list.empty())  // least recently used evictable page, with the nodes below it
      p->evictions += drop_subtree(p, p->evictable.begin()->second);
    const int id = p->free_list.back();
    p->free_list.pop_back();
    p->refs[id] = 1;
    out[i] = id;
  }
  return 0;
}

int mrsum_pages_free(void* h, int n, const int* ids) {
  auto* p = static_cast<Pages*>(h);
  std::lock_guard<std::mutex> g(p->mu);
  return release_locked(p, n, ids);
}

int mrsum_pages_release(void* h, int n, const int* ids) { return mrsum_pages_free(h, n, ids); }

int mrsum_pages_available(void* h) {
  auto* p = static_cast<Pages*>(h);
  std::lock_guard<std::mutex> g(p->mu);
  return static_cast<int>(p->free_list.size() + p->evictable.size());
}

int mrsum_pages_match(void* h, const int* toks, int n_toks, int* out) {
  auto* p = static_cast<Pages*>(h);
  std::lock_guard<std::mutex> g(p->mu);
  const int cap = n_toks > 0 ? (n_toks - 1) / PAGE_TOKENS : 0;
  int n = 0, parent = -1;
  while (n < cap) {
    const int id = find_node(p, parent, toks + static_cast<size_t>(n) * PAGE_TOKENS);
    if (id < 0) break;
    out[n++] = parent = id;
  }
  for (int i = n - 1; i >= 0; --i) {  // leaf first: the head of a chain is its most recent page
    const int id = out[i];
    if (p->refs[id]++ == 0) p->evictable.erase({p->tick[id], id});
    p->tick[id] = ++p->clock;
  }
  return n;
}

int mrsum_pages_publish(void* h, const int* toks, int n_toks, const int* pages, int n_full) {
  auto* p = static_cast<Pages*>(h);
  std::lock_guard<std::mutex> g(p->mu);
  const int total = static_cast<int>(p->refs.size());
  if (n_full < 0 || static_cast<long long>(n_full) * PAGE_TOKENS > n_toks) return -1;
  for (int i = 0; i < n_full; ++i)
    if (pages[i] < p->reserved || pages[i] >= total || p->refs[pages[i]] <= 0) return -1;
  if (p->toks.empty() && n_full) p->toks.assign(static_cast<size_t>(total) * PAGE_TOKENS, 0);
  std::vector<int> chain;
  int parent = -1, added = 0;
  for (int i = 0; i < n_full; ++i) {
    const int32_t* t = toks + static_cast<size_t>(i) * PAGE_TOKENS;
    int id = find_node(p, parent, t);
    if (id < 0) {
      id = pages[i];
      if (p->cached[id]) break;  // the caller's page is another chain's node already: stop here
      std::memcpy(&p->toks[static_cast<size_t>(id) * PAGE_TOKENS], t, PAGE_TOKENS * sizeof(int32_t));
      p->cached[id] = 1;
      p->parent[id] = parent;
      if (parent >= 0) p->kids[parent].push_back(id);
      p->by_hash.emplace(node_hash(parent, t), id);
      ++p->n_cached;
      ++added;
    }
    chain.push_back(id);
    parent = id;
  }
  for (size_t i = chain.size(); i-- > 0;) touch(p, chain[i]);
  return added;
}

void mrsum_pages_reset(void* h) {
  auto* p = static_cast<Pages*>(h);
  std::lock_guard<std::mutex> g(p->mu);
  for (int id = static_cast<int>(p->refs.size()) - 1; id >= p->reserved; --id)
    if (p->cached[id]) {
      p->kids[id].clear();
      drop_node(p, id, false);
    }
}

int mrsum_pages_cached(void* h) {
  auto* p = static_cast<Pages*>(h);
  std::lock_guard<std::mutex> g(p->mu);
  return p->n_cached;
}

long long mrsum_pages_evictions(void* h) {
  auto* p = static_cast<Pages*>(h);
  std::lock_guard<std::mutex> g(p->mu);
  return p->evictions;
}

void mrsum_pages_destroy(void* h) { delete static_cast<Pages*>(h); }

}  // extern "C"
