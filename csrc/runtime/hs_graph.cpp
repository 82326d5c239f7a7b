// Captured HIP graphs of query pipelines with per-replay kernel arguments.
//
// A fused query pipeline (exec/graphs.py: range search + tile map + generated scan kernel +
// result fold; or the two-phase merge join's tags + candidate scan + result fold) is captured
// once from a stream and replayed per query.  Every node is a kernel: the fold writes the result
// into the replay's pinned host block, whose address travels in its argument struct, and the
// range bounds travel in the search kernel's.  The generated kernels take their literals
// in a by-value argument struct (kernarg segment): reading that struct from device memory instead
// would turn every column load of the kernel into a flat load (the compiler cannot prove a pointer
// read from memory is global), which measured ~2x slower on gfx950.  So instead of a parameter
// copy node, each replay rewrites the argument blocks of the captured kernel nodes
// (hipGraphExecKernelNodeSetParams) and launches the executable graph.
//
// C ABI (ctypes, hyperspace_amd/exec/graphs.py):
//   hs_graph_capture_begin(stream)
//   hs_graph_capture_end(stream, funcs, nfuncs) -> handle   (kernel node i = first node of funcs[i])
//   hs_graph_set_args(handle, i, args, size)                 (next launches use these arguments)
//   hs_graph_launch(handle, stream)
//   hs_graph_replay(handle, nblocks, blocks, stream, after, done)
//       one query's replay in one call: optionally order ``stream`` after ``after``'s queued
//       work, rewrite the first nblocks kernel nodes' argument blocks, launch, and record the
//       slot's ``done`` event (the Python side's per-call overhead was several torch stream /
//       event calls per query)
//   hs_graph_clone(handle) -> handle       (another executable graph of the same capture)
//   hs_graph_node_counts(handle, &kernels, &memcpys, &others)
//   hs_graph_destroy(handle)
//   funcs[i] is a generated kernel's hipFunction_t or a library kernel's function address
//   (hs_agg_fold_func / hs_range_search_val_func of libhs_kernels: ONE by-value struct each).
//   hs_event_create() / hs_event_record(ev, stream) / hs_event_query(ev) / hs_event_sync(ev) /
//   hs_event_destroy(ev)       (timing-disabled events of the replay slots)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace {

thread_local std::string g_err;

struct HsGraph {
  // the captured graph: shared by the handle of the capture and its clones (hs_graph_clone),
  // destroyed with the last of them
  std::shared_ptr<ihipGraph> graph;
  hipGraphExec_t exec = nullptr;
  hipEvent_t join = nullptr;               // hs_graph_replay's ``after`` ordering event
  std::vector<hipGraphNode_t> nodes;       // the kernel node of funcs[i]
  std::vector<hipKernelNodeParams> params;  // its captured launch configuration
};

int fail(const char* what, hipError_t e) {
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return (int)e;
}

// Sorts ``all`` into dependency order: every node after the nodes it depends on (hipGraphGetNodes
// promises no order).  Two kernel nodes of one function - the pair pipeline's two phase-2
// launches - are then taken by hs_graph_capture_end in the order the captured chain runs them.
bool sort_by_depth(std::vector<hipGraphNode_t>& all) {
  const size_t n = all.size();
  std::vector<std::vector<size_t>> deps(n);
  for (size_t k = 0; k < n; ++k) {
    size_t nd = 0;
    if (hipGraphNodeGetDependencies(all[k], nullptr, &nd) != hipSuccess) return false;
    std::vector<hipGraphNode_t> d(nd);
    if (nd && hipGraphNodeGetDependencies(all[k], d.data(), &nd) != hipSuccess) return false;
    for (size_t j = 0; j < nd; ++j) {
      size_t at = 0;
      while (at < n && all[at] != d[j]) ++at;
      if (at == n) return false;
      deps[k].push_back(at);
    }
  }
  std::vector<int> depth(n, -1);   // longest chain of dependencies below the node
  for (size_t done = 0, pass = 0; done < n; ++pass) {
    if (pass > n) return false;    // (a cycle: not a captured graph)
    for (size_t k = 0; k < n; ++k) {
      if (depth[k] >= 0) continue;
      int d = 0;
      for (size_t j : deps[k]) {
        if (d < 0 || depth[j] < 0) {
          d = -1;   // a dependency not placed yet: next pass
        } else if (depth[j] + 1 > d) {
          d = depth[j] + 1;
        }
      }
      if (d >= 0) {
        depth[k] = d;
        ++done;
      }
    }
  }
  std::vector<size_t> idx(n);
  for (size_t k = 0; k < n; ++k) idx[k] = k;
  std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return depth[a] < depth[b]; });
  std::vector<hipGraphNode_t> out(n);
  for (size_t k = 0; k < n; ++k) out[k] = all[idx[k]];
  all.swap(out);
  return true;
}

}  // namespace

extern "C" {

const char* hs_graph_last_error() { return g_err.c_str(); }

int hs_graph_capture_begin(void* stream) {
  const hipError_t e = hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal);
  return e == hipSuccess ? 0 : fail("hipStreamBeginCapture", e);
}

// Ends the capture and instantiates.  funcs[i] (hipFunction_t of a generated kernel) names the
// kernel node whose arguments hs_graph_set_args(.., i, ..) rewrites: the first captured kernel
// node, in dependency order, launching that function and not already taken.  Returns nullptr on
// failure.
void* hs_graph_capture_end(void* stream, void** funcs, int nfuncs) {
  hipGraph_t graph = nullptr;
  hipError_t e = hipStreamEndCapture((hipStream_t)stream, &graph);
  if (e != hipSuccess || graph == nullptr) {
    fail("hipStreamEndCapture", e);
    return nullptr;
  }
  auto* g = new HsGraph();
  g->graph = std::shared_ptr<ihipGraph>(graph, [](hipGraph_t x) { hipGraphDestroy(x); });
  size_t n = 0;
  e = hipGraphGetNodes(graph, nullptr, &n);
  std::vector<hipGraphNode_t> all(n);
  if (e == hipSuccess && n) e = hipGraphGetNodes(graph, all.data(), &n);
  if (e != hipSuccess) {
    fail("hipGraphGetNodes", e);
    delete g;
    return nullptr;
  }
  all.resize(n);
  if (!sort_by_depth(all)) {
    g_err = "hs_graph_capture_end: could not order the captured nodes by dependency";
    delete g;
    return nullptr;
  }
  std::vector<char> taken(n, 0);
  for (int i = 0; i < nfuncs; ++i) {
    bool found = false;
    for (size_t k = 0; k < n && !found; ++k) {
      if (taken[k]) continue;
      hipGraphNodeType t;
      if (hipGraphNodeGetType(all[k], &t) != hipSuccess || t != hipGraphNodeTypeKernel) continue;
      hipKernelNodeParams p;
      std::memset(&p, 0, sizeof(p));
      if (hipGraphKernelNodeGetParams(all[k], &p) != hipSuccess) continue;
      if (p.func != funcs[i]) continue;
      taken[k] = 1;
      g->nodes.push_back(all[k]);
      g->params.push_back(p);
      found = true;
    }
    if (!found) {
      g_err = "hs_graph_capture_end: kernel node of function " + std::to_string(i) + " not found";
      delete g;
      return nullptr;
    }
  }
  e = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    fail("hipGraphInstantiate", e);
    delete g;
    return nullptr;
  }
  return g;
}

// Another executable graph of ``handle``'s captured graph: same node table, no second capture.
// The clone replays independently of the original (its own argument blocks per replay), so one
// capture serves every in-flight instance of a pipeline.  Returns nullptr on failure.
void* hs_graph_clone(void* handle) {
  auto* src = (HsGraph*)handle;
  if (src == nullptr || !src->graph) {
    g_err = "hs_graph_clone: no captured graph";
    return nullptr;
  }
  auto* g = new HsGraph();
  g->graph = src->graph;
  g->nodes = src->nodes;
  g->params = src->params;
  const hipError_t e = hipGraphInstantiate(&g->exec, g->graph.get(), nullptr, nullptr, 0);
  if (e != hipSuccess) {
    fail("hipGraphInstantiate", e);
    delete g;
    return nullptr;
  }
  return g;
}

// Node counts of the captured graph by kind (tests: a pipeline is kernel nodes only).
int hs_graph_node_counts(void* handle, int* kernels, int* memcpys, int* others) {
  auto* g = (HsGraph*)handle;
  size_t n = 0;
  hipError_t e = hipGraphGetNodes(g->graph.get(), nullptr, &n);
  std::vector<hipGraphNode_t> all(n);
  if (e == hipSuccess && n) e = hipGraphGetNodes(g->graph.get(), all.data(), &n);
  if (e != hipSuccess) return fail("hipGraphGetNodes", e);
  int nk = 0, nm = 0, no = 0;
  for (size_t k = 0; k < n; ++k) {
    hipGraphNodeType t;
    e = hipGraphNodeGetType(all[k], &t);
    if (e != hipSuccess) return fail("hipGraphNodeGetType", e);
    if (t == hipGraphNodeTypeKernel) ++nk;
    else if (t == hipGraphNodeTypeMemcpy) ++nm;
    else ++no;
  }
  *kernels = nk;
  *memcpys = nm;
  *others = no;
  return 0;
}

// Kernel node i of the executable graph takes the argument block ``args`` (the generated kernels
// have ONE by-value struct parameter, so kernelParams = {args}) from its next launch on.
int hs_graph_set_args(void* handle, int i, void* args, size_t size) {
  auto* g = (HsGraph*)handle;
  if (i < 0 || (size_t)i >= g->nodes.size()) {
    g_err = "hs_graph_set_args: bad node index";
    return -1;
  }
  (void)size;
  hipKernelNodeParams p = g->params[i];
  void* kp[1] = {args};
  p.kernelParams = kp;
  p.extra = nullptr;
  const hipError_t e = hipGraphExecKernelNodeSetParams(g->exec, g->nodes[i], &p);
  return e == hipSuccess ? 0 : fail("hipGraphExecKernelNodeSetParams", e);
}

int hs_graph_launch(void* handle, void* stream) {
  auto* g = (HsGraph*)handle;
  const hipError_t e = hipGraphLaunch(g->exec, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail("hipGraphLaunch", e);
}

int hs_graph_replay(void* handle, int nblocks, void** blocks, void* stream, void* after,
                    void* done) {
  auto* g = (HsGraph*)handle;
  if (nblocks < 0 || (size_t)nblocks > g->nodes.size()) {
    g_err = "hs_graph_replay: bad block count";
    return -1;
  }
  hipError_t e;
  if (after != nullptr && after != stream) {
    if (g->join == nullptr) {
      e = hipEventCreateWithFlags(&g->join, hipEventDisableTiming);
      if (e != hipSuccess) return fail("hipEventCreateWithFlags", e);
    }
    e = hipEventRecord(g->join, (hipStream_t)after);
    if (e != hipSuccess) return fail("hipEventRecord", e);
    e = hipStreamWaitEvent((hipStream_t)stream, g->join, 0);
    if (e != hipSuccess) return fail("hipStreamWaitEvent", e);
  }
  for (int i = 0; i < nblocks; ++i) {
    if (blocks[i] == nullptr) continue;
    hipKernelNodeParams p = g->params[i];
    void* kp[1] = {blocks[i]};
    p.kernelParams = kp;
    p.extra = nullptr;
    e = hipGraphExecKernelNodeSetParams(g->exec, g->nodes[i], &p);
    if (e != hipSuccess) return fail("hipGraphExecKernelNodeSetParams", e);
  }
  e = hipGraphLaunch(g->exec, (hipStream_t)stream);
  if (e != hipSuccess) return fail("hipGraphLaunch", e);
  if (done != nullptr) {
    e = hipEventRecord((hipEvent_t)done, (hipStream_t)stream);
    if (e != hipSuccess) return fail("hipEventRecord", e);
  }
  return 0;
}

void* hs_event_create() {
  hipEvent_t ev = nullptr;
  const hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e != hipSuccess) {
    fail("hipEventCreateWithFlags", e);
    return nullptr;
  }
  return ev;
}

int hs_event_record(void* ev, void* stream) {
  const hipError_t e = hipEventRecord((hipEvent_t)ev, (hipStream_t)stream);
  return e == hipSuccess ? 0 : fail("hipEventRecord", e);
}

// 0: complete, 1: not ready, < 0: error
int hs_event_query(void* ev) {
  const hipError_t e = hipEventQuery((hipEvent_t)ev);
  if (e == hipSuccess) return 0;
  if (e == hipErrorNotReady) return 1;
  return -fail("hipEventQuery", e);
}

int hs_event_sync(void* ev) {
  const hipError_t e = hipEventSynchronize((hipEvent_t)ev);
  return e == hipSuccess ? 0 : fail("hipEventSynchronize", e);
}

void hs_event_destroy(void* ev) {
  if (ev != nullptr) hipEventDestroy((hipEvent_t)ev);
}

void hs_graph_destroy(void* handle) {
  auto* g = (HsGraph*)handle;
  if (g == nullptr) return;
  if (g->join) hipEventDestroy(g->join);
  if (g->exec) hipGraphExecDestroy(g->exec);
  delete g;   // (the captured graph goes with its last handle)
}

}  // extern "C"
