// 32 bit symbols: rle32_{sym,byte}[_packed], rle32_{3,7}symlut_{sym,byte}  (reference: src/rle.h)
#define HSRLE_S 4
#include "hsrle_inst_generic.inc"
namespace hsrle { void register_w32(CodecLaunch *t) { register_width(t); } }
