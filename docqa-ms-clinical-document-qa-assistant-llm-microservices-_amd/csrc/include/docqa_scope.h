// docqa_scope.h -- the row-scope predicate shared by the scoped exact search (knn.hip) and
// the lexical scan (lexical.hip).
#pragma once
#include "docqa_common.h"

namespace docqa {

// The scope predicate (the fp32 reference ops/reference.py knn_scoped states the same):
//   row_tag == alt_tag || ((tag < 0 || row_tag == tag) && day_lo <= row_day && row_day <= day_hi)
// s = (tag, alt_tag, day_lo, day_hi).  tag -1 = any tag; alt_tag -1 = none (row tags are
// >= 0), 0 = also the knowledge base, exempt from the window; (INT32_MIN, INT32_MAX) = no
// window; an undated row carries day INT32_MIN, so any real bound excludes it.
__device__ __forceinline__ bool scope_match(const int4 s, int row_tag, int row_day) {
  return row_tag == s.y || ((s.x < 0 || row_tag == s.x) && s.z <= row_day && row_day <= s.w);
}

}  // namespace docqa
