// 16 bit symbols: rle16_{sym,byte}[_packed], rle16_{3,7}symlut_{sym,byte}  (reference: src/rle.h)
#define HSRLE_S 2
#include "hsrle_inst_generic.inc"
namespace hsrle { void register_w16(CodecLaunch *t) { register_width(t); } }
