/*
 * gram.hip -- the Gram record's kernel and its launcher (gram_kernels.h; include/gdg.h, GRAM): an object of its own, since it is the one
 * kernel of the library on the matrix cores and nothing of io.hip's is needed to compile it.
 */
#include "../../include/gdg.h"
#include "gdg_internal.h"
#include "blend.h"
#include "gram_kernels.h"
