// 64 bit symbols: rle64_{sym,byte}[_packed], rle64_{3,7}symlut_{sym,byte}  (reference: src/rle.h)
#define HSRLE_S 8
#include "hsrle_inst_generic.inc"
namespace hsrle { void register_w64(CodecLaunch *t) { register_width(t); } }
