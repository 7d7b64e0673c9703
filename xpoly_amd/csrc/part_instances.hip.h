// The template instances that cross the library's sources. Each is compiled in ONE source (its explicit instantiation
// definition: X_ = `template`, or empty where the macro writes the keyword) and only declared in the sources that call
// it (X_ = `extern template` / `extern`), so that its kernels are compiled once. A source names the macros it needs
// inside namespace xpg, behind the headers that declare the templates.
//
//   instance                                   defined in     declared in
//   batch_dev<S>                 (k_batch)     api_six.hip    api_mip.hip (the controller's node batches, has_solution's LPs),
//                                                             api_batch_hbm.hip (LPs that do fit LDS), api_mip_hbm.hip (the controller's header)
//   six_batch_vc_dev / _host<S>  (k_six_batch_vc, six_solve)
//                                              api_six.hip    api_six_vc_hbm.hip (shapes that do fit 64 KB, a general vc)
//   mip_batch_device<S> (k_mip_tree), mip_batch_vc_host<S> (the host controller)
//                                              api_mip.hip    api_mip_hbm.hip (trees that do fit 64 KB, a general vc)
//   mip_tree_launch<R32>         (THE launch of k_mip_tree)
//                                              api_mip.hip    api_has_solution.hip (the integer form runs the walk twice)
#pragma once

#define XPG_BATCH_DEV(X_, S_) \
    X_ int batch_dev<S_>(xpg_ctx *, int, int, const S_ *, const S_ *, int, int, unsigned, int32_t *, S_ *, S_ *, uint32_t *, int);

#define XPG_SIX_VC_INSTANCES(X_, S_) \
    X_ int six_batch_vc_dev<S_>(xpg_ctx *, bool, int, const S_ *, const S_ *, const S_ *, int, const S_ *, int, int, unsigned, int, int32_t *, S_ *, S_ *); \
    X_ int six_batch_vc_host<S_>(xpg_ctx *, int, bool, int, const S_ *, const S_ *, const S_ *, int, const S_ *, int, int, unsigned, int32_t *, S_ *, S_ *);

#define XPG_MIP_SHARED(X_, S_) \
    X_ template int mip_batch_device<S_>(xpg_ctx *, int, bool, bool, const S_ *, const S_ *, int, int, int32_t *, S_ *, S_ *, long long *, \
                                         const uint8_t *, const S_ *, int, const int *, int); \
    X_ template int mip_batch_vc_host<S_>(xpg_ctx *, int, int, bool, bool, const S_ *, const S_ *, const S_ *, int, const S_ *, int, int, \
                                          const uint8_t *, int32_t *, S_ *, S_ *, long long *);

#define XPG_MIP_TREE_LAUNCH(X_, S_) \
    X_ template int mip_tree_launch<S_>(xpg_ctx *, const MipGeom &, int, int, const void *, const void *, int, int, bool, bool, int, int, void *, \
                                        size_t, void *, void *, void *, void *, const void *, const void *, const void *, const void *, int, void *, \
                                        const void *, int);
