// 24 bit symbols: rle24_{sym,byte}[_packed], rle24_{3,7}symlut_{sym,byte}  (reference: src/rle.h)
#define HSRLE_S 3
#include "hsrle_inst_generic.inc"
namespace hsrle { void register_w24(CodecLaunch *t) { register_width(t); } }
