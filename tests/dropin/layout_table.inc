// layout_table.inc -- the table of the drop-in check, printed by tu_reference_caller.cpp: in tests/test_dropin_cpu.py as
// fealess_amd/cadreco/fealess_cadreco.h defines the types, and as the reference's own CadReco/lotus_common.h +
// obj_reco_temp.h define them when tests/golden/make_golden.py --reference records tests/golden/cadreco_reference_abi.txt
// (by path, nothing copied).  It records sizeof / offsetof of every type that crosses the facade and the vtable slot of
// every virtual method of CObjRecoCAD.
#include <cstddef>
#include <cstring>
// Itanium C++ ABI: a pointer to a virtual member function holds 1 + the function's byte offset in the vtable
template <class F> static long long lt_vslot(F f)
{
  struct { long long ptr, adj; } r;
  static_assert(sizeof(F) == sizeof(r), "Itanium C++ ABI member function pointer");
  std::memcpy(&r, &f, sizeof r);
  return (r.ptr & 1) ? (r.ptr - 1) / (long long)sizeof(void *) : -1;
}
#define LT_ROW(name, value) { name, (long long)(value) }
static const struct { const char *name; long long value; } LAYOUT_TABLE[] = {
  LT_ROW("sizeof(TImageU)", sizeof(TImageU)),
  LT_ROW("offsetof(TImageU,dTimestamp)", offsetof(TImageU, dTimestamp)),
  LT_ROW("offsetof(TImageU,pData)", offsetof(TImageU, pData)),
  LT_ROW("offsetof(TImageU,nWidth)", offsetof(TImageU, nWidth)),
  LT_ROW("offsetof(TImageU,nHeight)", offsetof(TImageU, nHeight)),
  LT_ROW("sizeof(TImageU16)", sizeof(TImageU16)),
  LT_ROW("offsetof(TImageU16,pData)", offsetof(TImageU16, pData)),
  LT_ROW("sizeof(TImageF)", sizeof(TImageF)),
  LT_ROW("sizeof(TCamIntrinsicParam)", sizeof(TCamIntrinsicParam)),
  LT_ROW("offsetof(TCamIntrinsicParam,nWidth)", offsetof(TCamIntrinsicParam, nWidth)),
  LT_ROW("offsetof(TCamIntrinsicParam,nHeight)", offsetof(TCamIntrinsicParam, nHeight)),
  LT_ROW("offsetof(TCamIntrinsicParam,dFx)", offsetof(TCamIntrinsicParam, dFx)),
  LT_ROW("offsetof(TCamIntrinsicParam,dFy)", offsetof(TCamIntrinsicParam, dFy)),
  LT_ROW("offsetof(TCamIntrinsicParam,dCx)", offsetof(TCamIntrinsicParam, dCx)),
  LT_ROW("offsetof(TCamIntrinsicParam,dCy)", offsetof(TCamIntrinsicParam, dCy)),
  LT_ROW("offsetof(TCamIntrinsicParam,vdDistCoeff)", offsetof(TCamIntrinsicParam, vdDistCoeff)),
  LT_ROW("sizeof(Mat4x4F)", sizeof(Mat4x4F)),
  LT_ROW("sizeof(TObjRecoResult)", sizeof(TObjRecoResult)),
  LT_ROW("offsetof(TObjRecoResult,strObjTag)", offsetof(TObjRecoResult, strObjTag)),
  LT_ROW("offsetof(TObjRecoResult,tWorld2Cam)", offsetof(TObjRecoResult, tWorld2Cam)),
  LT_ROW("sizeof(TScanFrame)", sizeof(TScanFrame)),
  LT_ROW("offsetof(TScanFrame,tMask)", offsetof(TScanFrame, tMask)),
  LT_ROW("offsetof(TScanFrame,tWorld2Cam)", offsetof(TScanFrame, tWorld2Cam)),
  LT_ROW("offsetof(TScanFrame,tDepthImg)", offsetof(TScanFrame, tDepthImg)),
  LT_ROW("sizeof(TScanPackage)", sizeof(TScanPackage)),
  LT_ROW("offsetof(TScanPackage,tGLPrjMatrix)", offsetof(TScanPackage, tGLPrjMatrix)),
  LT_ROW("offsetof(TScanPackage,bounding_box)", offsetof(TScanPackage, bounding_box)),
  LT_ROW("offsetof(TScanPackage,vtScanFrame)", offsetof(TScanPackage, vtScanFrame)),
  LT_ROW("sizeof(AdvancedParam)", sizeof(AdvancedParam)),
  LT_ROW("sizeof(TTrainParam)", sizeof(TTrainParam)),
  LT_ROW("offsetof(TTrainParam,img_physical_width)", offsetof(TTrainParam, img_physical_width)),
  LT_ROW("sizeof(CObjRecoCAD)", sizeof(CObjRecoCAD)),
  LT_ROW("vslot(CObjRecoCAD::Train)", lt_vslot(&CObjRecoCAD::Train)),
  LT_ROW("vslot(CObjRecoCAD::AddObj)", lt_vslot(&CObjRecoCAD::AddObj)),
  LT_ROW("vslot(CObjRecoCAD::ClearObj)", lt_vslot(&CObjRecoCAD::ClearObj)),
  LT_ROW("vslot(CObjRecoCAD::SetROI)", lt_vslot(&CObjRecoCAD::SetROI)),
  LT_ROW("vslot(CObjRecoCAD::Recognition)", lt_vslot(&CObjRecoCAD::Recognition)),
  LT_ROW("vslot(CObjRecoCAD::SetAdvancedParam)", lt_vslot(&CObjRecoCAD::SetAdvancedParam)),
  LT_ROW("vslot(CObjRecoCAD::GetAdvancedParam)", lt_vslot(&CObjRecoCAD::GetAdvancedParam)),
  LT_ROW("EObjReco_LmICP", CObjRecoCAD::EObjReco_LmICP),
  LT_ROW("EObjReco_PoseNet", CObjRecoCAD::EObjReco_PoseNet),
  LT_ROW("ERROR_INVALID_PARAM", (int)ERROR_INVALID_PARAM),
  LT_ROW("ERROR_OPEN_FILE_FAILED", (int)ERROR_OPEN_FILE_FAILED),
  LT_ROW("ERROR_UNKNOW", (int)ERROR_UNKNOW),
};
