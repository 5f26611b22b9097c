// qg_build_id.hip -- qg_build_id(): the hash of every source the library is built from, which the Makefile passes in.  A translation
// unit of its own, so that an edit anywhere recompiles this one line and the edited unit, not the step kernels.
#ifndef QG_SOURCE_HASH
#define QG_SOURCE_HASH "unknown"
#endif
extern "C" const char *qg_build_id(void) { return QG_SOURCE_HASH; }
