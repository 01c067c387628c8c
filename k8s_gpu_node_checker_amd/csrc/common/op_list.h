// What the entry points of the instruction-level diagnostics decide about their arguments before anything is
// launched: whether a list of ops is one of the table, whether the self-check hook names a listed op and lies inside
// the grid, which of the two hooks a launch carries, and the record no launch has written yet.  The helpers decide;
// the caller words the refusal and picks the return code.
//
// Plain C++17, no HIP: the host compiler builds it alone (tests/test_op_list_cpu.py).
#ifndef K8S_GPU_NODE_CHECKER_AMD_OP_LIST_H_
#define K8S_GPU_NODE_CHECKER_AMD_OP_LIST_H_

#include <cstddef>
#include <vector>

// "known": ops[0..nops) is a list of 1..table_len indices into a table of table_len ops, with no index twice when
// `distinct`.
inline bool op_list_known(const int* ops, int nops, int table_len, bool distinct) {
  if (ops == nullptr || nops < 1 || nops > table_len) return false;
  std::vector<char> seen(static_cast<size_t>(table_len), 0);
  for (int i = 0; i < nops; ++i) {
    if (ops[i] < 0 || ops[i] >= table_len || (distinct && seen[ops[i]])) return false;
    seen[ops[i]] = true;
  }
  return true;
}

// "hook listed": inject_op is off (below 0) or one of ops[0..nops)
inline bool op_list_has_hook(const int* ops, int nops, int inject_op) {
  if (inject_op < 0) return true;
  for (int i = 0; ops != nullptr && i < nops; ++i)
    if (ops[i] == inject_op) return true;
  return false;
}

// the hook's range: its workgroup inside the grid, its skipped step (below 0: the flip) below `limit`
inline bool hook_in_range(int block, unsigned grid, int skip, int limit) {
  return block >= 0 && static_cast<unsigned>(block) < grid && skip < limit;
}

// What one launch is told of the hooks (-1: nothing): the flip acts when the skipped step is below 0, the skip otherwise.
struct HookTrio {
  int flip_block, skip_block, skip_at;
};
inline HookTrio hook_trio(bool hooked, int block, int skip) {
  return {hooked && skip < 0 ? block : -1, hooked && skip >= 0 ? block : -1, hooked ? skip : -1};
}

// "no record yet": where = ~0, the index, got and want 0
inline void no_record(unsigned long long* rec) {
  rec[0] = ~0ULL;
  rec[1] = rec[2] = rec[3] = 0;
}

#endif  // K8S_GPU_NODE_CHECKER_AMD_OP_LIST_H_
