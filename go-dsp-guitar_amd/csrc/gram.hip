/*
 * gram.hip -- the Gram record's kernel and its launcher (gram_kernels.h; include/gdg.h, GRAM): an object of its own, since it was the first
 * kernel of the library on the matrix cores and nothing of io.hip's is needed to compile it.  Behind it the tap-fit record's, the same
 * instruction over shifted copies of a row (tapfit_kernels.h; include/gdg.h, TAPFIT).
 */
#include "../../include/gdg.h"
#include "gdg_internal.h"
#include "blend.h"
#include "gram_kernels.h"
#include "tapfit_kernels.h"
