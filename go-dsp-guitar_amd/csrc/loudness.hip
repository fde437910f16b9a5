/*
 * loudness.hip -- the loudness records' kernel and its launcher (loudness_kernels.h; include/gdg.h, LOUDNESS): an object of its own, on a path
 * of its own beside the block records of io.hip, fir.hip and gram.hip; nothing of theirs is needed to compile it.
 */
#include "../../include/gdg.h"
#include "gdg_internal.h"
#include "loudness_kernels.h"
