/*
 * makani_amd.h -- C ABI of the MI355X-native SFNO spectral hot path.
 *
 * One shared library (libmakani_amd.so, built by hipcc for gfx950) exports the
 * entry points below.  Plain pointers and sizes only; every device pointer is a
 * HIP device address, every `stream` is a hipStream_t passed as void*.  All
 * kernels are launched asynchronously on `stream` (graph-capturable: no
 * allocation, no host synchronisation inside).  Return value: 0 on success,
 * non-zero on error (mk_last_error() holds the message for the calling thread).
 *
 * The reference (choutilin/makani) has no FFI: its hot path is PyTorch ops
 * behind nn.Module interfaces.  Each entry point names the reference call it
 * replaces (file:line under the reference tree); INTEGRATION.md shows the
 * ctypes binding a maintainer would add.
 *
 * Private device layouts (chosen for coalesced HBM access on CDNA4):
 *   grid field   x  [BC][K][N]      real fp32, N contiguous      (= NCHW, B*C flattened)
 *   Fourier rows xf [M][K][BC]      complex64 interleaved, BC contiguous ("MKBC")
 *   spectrum     c  [L][M][BC]      complex64 interleaved, BC contiguous ("LMBC")
 *   dhconv weight w [L][I][O]       complex64 interleaved, O contiguous
 *   Legendre tab    [M][L][KP]      fp32, KP = K rounded up to 32, zero padded
 * The public torch layout [B,C,L,M] complex64 is converted with mk_spec_pack /
 * mk_spec_unpack.
 */
#ifndef MAKANI_AMD_H
#define MAKANI_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library ---------------------------------------------------------- */
int mk_version(void);
const char* mk_last_error(void);

/* ---- host-side precompute (float64 arithmetic, no GPU needed) ---------- */
/* grid: 0 = "equiangular" (Clenshaw-Curtis), 1 = "legendre-gauss". */

/* Colatitudes (ascending from the north pole) and quadrature weights, nlat each.
 * Replaces torch_harmonics.quadrature.{clenshaw_curtiss,legendre_gauss}_weights
 * (reference call sites: makani/utils/grids.py:19,32,77,83; sfnonet.py:536-539). */
int mk_quadrature(int grid, int nlat, double* theta, double* weights);

/* Padded row length of the Legendre table for nlat latitudes. */
int mk_legendre_kpad(int nlat);

/* Orthonormal associated Legendre table with Condon-Shortley phase,
 * out[m][l][k] for m<mmax, l<lmax, k<kpad (zero for k>=nlat and l<m), fp32
 * rounded from float64.  with_quad_weights != 0 multiplies by w_k (forward
 * transform table, torch-harmonics RealSHT.weights); 0 gives the synthesis
 * table (InverseRealSHT.pct).  Replaces torch_harmonics.legendre._precompute_legpoly
 * as invoked by sfnonet.py:536-539. */
int mk_legendre_table(int grid, int nlat, int lmax, int mmax, int with_quad_weights, float* out);

/* Twiddle table for real FFTs of length nlon: out holds 2*(nlon/2) + 2*(nlon/2+1)
 * floats: exp(-2 pi i j/(nlon/2)) for j<nlon/2, then exp(-2 pi i m/nlon) for m<=nlon/2. */
int mk_fft_twiddle_len(int nlon);
int mk_fft_twiddles(int nlon, float* out);

/* ---- longitudinal real FFT (K1 / K4) ----------------------------------- */
/* xf[m][k][bc] = s_m * sum_n x[bc][k][n] exp(-2 pi i m n / nlon), m < mmax, with
 * s_0 = scale0, s_{nlon/2} = scale_h (Nyquist), s_m = scale_m otherwise.
 * Forward SHT uses all three = 2 pi / nlon:
 * `2*pi*torch.fft.rfft(x, dim=-1, norm="forward")[..., :mmax]` of torch-harmonics
 * RealSHT.forward (called at spectral_convolution.py:131, sfnonet.py:596).
 * With (1, 2, 1) it is the adjoint of mk_irfft(1, 1, 1) (backward of K4).
 * x_dtype: 0 = fp32, 1 = bf16 input rows. */
int mk_rfft(const void* x, int x_dtype, float* xf, const float* twiddles,
            int bc, int nlat, int nlon, int mmax, float scale0, float scale_m, float scale_h,
            void* stream);

/* x[bc][k][n] = s_0 Re(xf[0][k][bc]) + sum_{0<m<mmax, m != nlon/2} 2 s_m Re(xf[m][k][bc] exp(2 pi i m n/nlon))
 *               + s_h Re(xf[nlon/2][k][bc]) (-1)^n   (only if mmax == nlon/2+1).
 * (1, 1, 1) is `torch.fft.irfft(x, n=nlon, dim=-1, norm="forward")` of
 * InverseRealSHT.forward (spectral_convolution.py:133,141; sfnonet.py:598): modes
 * >= mmax are zero, imaginary parts of the zero and Nyquist modes are ignored.
 * With (2 pi/nlon, pi/nlon, 2 pi/nlon) it is the adjoint of mk_rfft (backward of K1).
 * x_dtype: 0 = fp32 rows out, 1 = bf16 rows out (fuses the `.to(dtype)` of
 * spectral_convolution.py:134,146; production lengths 480 / 1440 only). */
int mk_irfft(const float* xf, void* x, int x_dtype, const float* twiddles,
             int bc, int nlat, int nlon, int mmax, float scale0, float scale_m, float scale_h,
             void* stream);

/* ---- Legendre contraction on fp32 MFMA (K2 / K3) ------------------------ */
/* Analysis: c[l][m][n] = sum_k tab[m_off+m][l_off.. l][k] xf[m][k][n], n < 2*bc (re/im as
 * independent real columns), only l >= m (global indices); entries with l < m are not
 * written.  torch-harmonics `einsum('...kmr,mlk->...lmr', x, weights)`.
 * m_off: global index of local mode 0 (w-sharded tables); tab points at the
 * full [mmax_glob][lmax][kpad] table. */
int mk_legendre_fwd(const float* xf, const float* tab, float* c,
                    int bc, int nlat, int lmax, int mmax_loc, int m_off, int mmax_glob, void* stream);

/* Synthesis: xf[m][k][n] = sum_{l>=m} tab[m][l][k] c[l][m][n].
 * torch-harmonics `einsum('...lmr,mlk->...kmr', x, pct)`.  Also the backward of
 * mk_legendre_fwd (with the analysis table); mk_legendre_fwd with the synthesis
 * table is the backward of this one. */
int mk_legendre_inv(const float* c, const float* tab, float* xf,
                    int bc, int nlat, int lmax, int mmax_loc, int m_off, int mmax_glob, void* stream);

/* ---- the same contractions on the bf16 matrix cores, fp32-accurate ("bf16x3") ----------
 * Every fp32 operand is split exactly into three bf16 pieces and each product is evaluated
 * as the six leading piece products, accumulated in fp32 (error ~2^-22 relative, same
 * parity budget as above).  The table is pre-split once into the kernels' tile images:
 *   inverse = 0: for contractions over latitude  (mk_legendre_fwd_x3)
 *   inverse = 1: for contractions over degree    (mk_legendre_inv_x3)
 * mk_legendre_x3_bytes: size of the image; mk_legendre_x3_split: fp32 device table
 * [mmax][lmax][kpad] (mk_legendre_table) -> image (device). */
long long mk_legendre_x3_bytes(int nlat, int lmax, int mmax, int inverse);
int mk_legendre_x3_split(const float* tab, void* out, int nlat, int lmax, int mmax, int inverse, void* stream);
/* Same contracts as mk_legendre_fwd / mk_legendre_inv with `tab_x3` the matching image. */
int mk_legendre_fwd_x3(const float* xf, const void* tab_x3, float* c,
                       int bc, int nlat, int lmax, int mmax_loc, int m_off, int mmax_glob, void* stream);
int mk_legendre_inv_x3(const float* c, const void* tab_x3, float* xf,
                       int bc, int nlat, int lmax, int mmax_loc, int m_off, int mmax_glob, void* stream);

/* ---- latitude-major Fourier rows (distributed SHT) ---------------------------------------
 * `_ex` forms with xf_layout: 0 = xf[m][k][bc] (all calls above), 1 = xf[k][m][bc].  With latitude
 * outermost the two latitude all-to-alls of the distributed transform (makani/mpu/layers.py:38-169 pattern,
 * torch_harmonics distributed_transpose_polar) gather / split the OUTERMOST axis, so the received chunks are the
 * operand and the sent chunks lie back to back: no pack / concatenate copies on that side. */
int mk_rfft_ex(const void* x, int x_dtype, float* xf, const float* twiddles, int bc, int nlat, int nlon,
               int mmax, float scale0, float scale_m, float scale_h, int xf_layout, void* stream);
int mk_irfft_ex(const float* xf, void* x, int x_dtype, const float* twiddles, int bc, int nlat, int nlon,
                int mmax, float scale0, float scale_m, float scale_h, int xf_layout, void* stream);
int mk_legendre_fwd_x3_ex(const float* xf, const void* tab_x3, float* c, int bc, int nlat, int lmax,
                          int mmax_loc, int m_off, int mmax_glob, int xf_layout, void* stream);
int mk_legendre_inv_x3_ex(const float* c, const void* tab_x3, float* xf, int bc, int nlat, int lmax,
                          int mmax_loc, int m_off, int mmax_glob, int xf_layout, void* stream);

/* Peer-major Fourier rows for the distributed transform: bc = batch * chans rows, the channels cut into blocks of
 * chans_per_peer (a multiple of 24), xf = [chans / chans_per_peer][nlat][mmax][batch][chans_per_peer] -- exactly the send
 * (analysis) / receive (synthesis) buffer of the channel <-> latitude all-to-all, so that side of the transpose needs no
 * pack / concatenate copy either.  Production lengths only (nlon 480 / 1440, mmax <= 241). */
int mk_rfft_pm(const void* x, int x_dtype, float* xf, const float* twiddles, int bc, int nlat, int nlon, int mmax,
               float scale0, float scale_m, float scale_h, int chans, int chans_per_peer, void* stream);
int mk_irfft_pm(const float* xf, void* x, int x_dtype, const float* twiddles, int bc, int nlat, int nlon, int mmax,
                float scale0, float scale_m, float scale_h, int chans, int chans_per_peer, void* stream);

/* Inverse transform that also delivers the statistics of its output (round 3): rowsums[2 r], rowsums[2 r + 1] += sum and sum of
 * squares of output row r (= b * C + c) over this call's latitudes, on the values as stored; fp64 accumulators zeroed by the
 * caller.  It is the statistics pass of the instance norm that follows the inverse SHT in every FNO block
 * (sfnonet.py:239-253: norm0) without a second read of the field.  chans_per_peer > 0: peer-major rows as mk_irfft_pm, else
 * xf_layout as mk_irfft_ex.  Production lengths only (nlon 480 / 1440, mmax <= 241). */
int mk_irfft_sums(const float* xf, void* x, int x_dtype, const float* twiddles, int bc, int nlat, int nlon, int mmax,
                  float scale0, float scale_m, float scale_h, int xf_layout, int chans, int chans_per_peer, double* rowsums,
                  void* stream);
/* mk_irfft_sums with statistics that are float64 throughout and independent of scheduling: every latitude's share goes to
 * workspace[nlat][bc][2] (doubles, need not be zeroed) and a second launch adds the latitudes in a fixed order into
 * rowsums (+=, zeroed by the caller).  mk_irfft_sums itself adds each latitude's share rounded to fp32 with one atomic
 * (reproducible too, accurate to about 2^-24); the planar InverseRealFFT2.inverse_packed uses this entry. */
int mk_irfft_sums_ws(const float* xf, void* x, int x_dtype, const float* twiddles, int bc, int nlat, int nlon, int mmax,
                     float scale0, float scale_m, float scale_h, int xf_layout, int chans, int chans_per_peer, double* rowsums,
                     double* workspace, void* stream);
/* The same inverse transform with a companion field added in the store epilogue under a per-row affine map:
 *   x[r] = irfft(xf)[r] + affine[r][0] * z[r] + affine[r][1]     z, x: [bc][nlat][nlon] in x_dtype; affine fp32 [bc][2]
 * -- a skip connection synthesised from the (channel-mixed) spectrum plus the apply pass of the instance norm of z
 * (mk_instnorm_coeffs): the synthesised field is never written on its own.  Split kernels only (nlon 480 / 1440, mmax <= 241). */
int mk_irfft_affine_add(const float* xf, void* x, int x_dtype, const float* twiddles, int bc, int nlat, int nlon,
                        int mmax, float scale0, float scale_m, float scale_h, int xf_layout, const void* z,
                        const float* affine, void* stream);

/* ---- latitude DFT of the planar transform -------------------------------------------------------
 * RealFFT2 / InverseRealFFT2 (layers.py:219-287, selected by spectral_transform="fft" at sfnonet.py:541-555):
 * `rfft2(x, norm="ortho")` keeps mmax longitudinal modes and the first ceil(lmax / 2) and last floor(lmax / 2) latitude
 * frequencies.  The longitudinal part is mk_rfft_ex / mk_irfft_ex with all three scales 1 / sqrt(nlon) and xf_layout = 1;
 * the latitude part is a dense complex matrix, the same for every mode:
 *   W[l][k] = exp(-2 pi i f_l k / nlat) / sqrt(nlat),   f_l = l for l < ceil(lmax / 2), else nlat - lmax + l.
 * mk_latdft_table (host, float64 rounded once to fp32; the angle from f_l * k reduced modulo nlat in integers) writes
 * mk_latdft_table_len(nlat, lmax) floats: cos [lmax][KP], sin [lmax][KP] (W = cos - i sin), then the transposes
 * cos [nlat][LP], sin [nlat][LP] for the inverse; KP / LP = nlat / lmax rounded up to 4, zero padded.
 * Needs nlat >= 2, 2 <= lmax <= nlat (the length query returns 0 otherwise). */
long long mk_latdft_table_len(int nlat, int lmax);
int mk_latdft_table(int nlat, int lmax, float* out);
/* The same table (length, layout, rounding) over a contiguous WINDOW of frequencies, f_l = (first + l) mod nlat: the rows the
 * channels-last AFNO keeps (networks/afnonet.py:78-103: `total_modes - kept_modes : total_modes + kept_modes`, contiguous around
 * the Nyquist row, not RealFFT2's low frequencies).  mk_latdft_fwd / mk_latdft_inv take either table as data.  first = 0 and
 * lmax = nlat give mk_latdft_table's bits.  Needs 0 <= first < nlat and 2 <= lmax <= nlat. */
int mk_latdft_table_window(int nlat, int lmax, int first, float* out);
/* fwd: c[l][j]  = sum_k W[l][k] xf[k][j]            xf complex64 [nlat][ncols], c complex64 [lmax][ncols]
 * inv: xf[k][j] = sum_l conj(W[l][k]) c[l][j]       ncols = mmax_loc * bc; only the kept frequencies are contracted
 * (the zero padding between the high and the low modes of InverseRealFFT2.forward is implicit).  Each is the adjoint
 * (backward) of the other.  bf16x3 engine (fp32-accurate), no atomics; `table` (device copy of mk_latdft_table's
 * output) 16-byte aligned, 33 * 2 * ncols * 4 < 2^31. */
int mk_latdft_fwd(const float* xf, const float* table, float* c, int nlat, int lmax, long long ncols, void* stream);
int mk_latdft_inv(const float* c, const float* table, float* xf, int nlat, int lmax, long long ncols, void* stream);

/* ---- spectral filter contraction (K5) ---------------------------------- */
/* y[l][m][b][o] = sum_i x[l][m][b][i] * w[l][i][o]  (complex), for global m <= l.
 * Replaces _contract_dhconv `einsum("bixy,iox->boxy")` (contractions.py:130-136,
 * dispatched by factorizations.py:167-200, called at spectral_convolution.py:137).
 * l_off / m_off: global indices of local l = 0 / m = 0 (h / w sharding). */
int mk_dhconv_fwd(const float* x, const float* w, float* y, int lloc, int mloc, int batch,
                  int cin, int cout, int l_off, int m_off, void* stream);
/* gx[l][m][b][i] = sum_o gy[l][m][b][o] * conj(w[l][i][o]) */
int mk_dhconv_dgrad(const float* gy, const float* w, float* gx, int lloc, int mloc, int batch,
                    int cin, int cout, int l_off, int m_off, void* stream);
/* gw[l][i][o] = sum_{m<=l, b} conj(x[l][m][b][i]) * gy[l][m][b][o] */
int mk_dhconv_wgrad(const float* x, const float* gy, float* gw, int lloc, int mloc, int batch,
                    int cin, int cout, int l_off, int m_off, void* stream);

/* bf16x3 variants of the three dhconv kernels (see the Legendre section): same contracts,
 * cin and cout must be even (returns an error otherwise; the fp32 kernels take any size). */
int mk_dhconv_fwd_x3(const float* x, const float* w, float* y, int lloc, int mloc, int batch,
                     int cin, int cout, int l_off, int m_off, void* stream);
int mk_dhconv_dgrad_x3(const float* gy, const float* w, float* gx, int lloc, int mloc, int batch,
                       int cin, int cout, int l_off, int m_off, void* stream);
int mk_dhconv_wgrad_x3(const float* x, const float* gy, float* gw, int lloc, int mloc, int batch,
                       int cin, int cout, int l_off, int m_off, void* stream);

/* ---- real channel mix on the spectrum -------------------------------------------------------
 * A bias-free 1x1 convolution commutes with the spherical harmonic transform (linear, the same for every
 * channel): sht(W x) = W sht(x), isht(W c) = W isht(c).  A convolution that sits next to a transform
 * (the encoder's last one, nn.Conv2d(embed, embed, 1, bias=False) of layers.py:124-131; the outer skip of
 * the last block, sfnonet.py:223-234) is evaluated on the private spectrum instead of the grid:
 *   fwd:   y[l][m][b][o]  = sum_i W[o][i] x[l][m][b][i]        W fp32 real [cout][cin], the same for every l
 *   dgrad: gx[l][m][b][i] = sum_o W[o][i] gy[l][m][b][o]
 *   wgrad: gw[o][i]      += sum_{m<=l, b} re(gy[l][m][b][o] * conj(x[l][m][b][i]))   (atomic adds: caller zeroes gw)
 * for global m <= l only (entries with l < m are neither read nor written), l_off / m_off as for dhconv.
 * bf16x3 engine (fp32-accurate); cin, cout even, operands 16-byte aligned. */
int mk_spec_mix_fwd(const float* x, const float* w, float* y, int lloc, int mloc, int batch,
                    int cin, int cout, int l_off, int m_off, void* stream);
int mk_spec_mix_dgrad(const float* gy, const float* w, float* gx, int lloc, int mloc, int batch,
                      int cin, int cout, int l_off, int m_off, void* stream);
int mk_spec_mix_wgrad(const float* x, const float* gy, float* gw, int lloc, int mloc, int batch,
                      int cin, int cout, int l_off, int m_off, void* stream);

/* ---- complex channel MLP on the spectrum (the non-linear filter, SpectralAttention) -------------
 * One layer of spectral_convolution.py:367-374 on the private spectrum [L][M][B][C] complex64, rows (m <= l, b) as in dhconv
 * (entries with l < m are neither read nor written; l_off >= mmax: the dense planar spectrum), bf16x3 engine:
 *   fwd:   y[l][m][b][o]  = act(sum_i x[l][m][b][i] * w[l * ws][i][o] + bias[o])
 *   dgrad: gx[l][m][b][i] = (sum_o gy[l][m][b][o] * conj(w[l * ws][i][o])) * mask(a[l][m][b][i])
 *   wgrad: gw[l][i][o]    = sum_{m<=l, b} conj(x[l][m][b][i]) * gy[l][m][b][o]      (per_degree; without: also summed over l)
 *   bgrad: gb[o]          = sum_{l, m<=l, b} g[l][m][b][o]
 * w: complex [cin][cout] panels, one per degree (per_degree = 1: the dhconv layout [L][cin][cout]) or one for all degrees
 * (per_degree = 0).  bias: complex [cout] or NULL.  act: 0 none, 1 ReLU on the real part (the imaginary part passes), 2 ReLU on
 * both parts; bias and activation are applied in fp32 on the accumulator.  a: the saved activation OUTPUT of the layer whose
 * result this layer's input was ([L][M][B][cin], act its mode) or NULL for no mask; a component passes where the same
 * component of a is > 0 (relu' with relu'(0) = 0), in mode 1 every imaginary component passes.
 * The shared weight gradient contracts groups of consecutive degrees into partial panels in `workspace`
 * (mk_spec_cmlp_wgrad_workspace bytes, 16-byte aligned; 0 bytes: not needed) and adds them in ascending order; the bias gradient
 * sums rows, then degrees, in float64 in a fixed order (`workspace`: mk_spec_cmlp_bgrad_workspace bytes).  Neither uses
 * atomics: the same bits on every run.  cin, cout even, operands 16-byte aligned, one degree of a field below 2^31 bytes. */
int mk_spec_cmlp_fwd(const float* x, const float* w, const float* bias, float* y, int lloc, int mloc, int batch, int cin,
                     int cout, int l_off, int m_off, int per_degree, int act, void* stream);
int mk_spec_cmlp_dgrad(const float* gy, const float* w, const float* a, float* gx, int lloc, int mloc, int batch, int cin,
                       int cout, int l_off, int m_off, int per_degree, int act, void* stream);
long long mk_spec_cmlp_wgrad_workspace(int lloc, int cin, int cout, int per_degree);
int mk_spec_cmlp_wgrad(const float* x, const float* gy, float* gw, void* workspace, int lloc, int mloc, int batch, int cin,
                       int cout, int l_off, int m_off, int per_degree, void* stream);
long long mk_spec_cmlp_bgrad_workspace(int lloc, int cout);
int mk_spec_cmlp_bgrad(const float* g, float* gb, void* workspace, int lloc, int mloc, int batch, int cout, int l_off,
                       int m_off, void* stream);

/* ---- block-diagonal complex MLP on the dense planar spectrum (AFNO2D, afnonet_v2.py:84-106) -----
 * The spectrum of RealFFT2.forward_packed is dense (no triangle) and is taken as flat rows r < rows = L * M * B of nb * ib
 * (nb * ob) complex64 channels, cut into nb blocks with one complex [ib][ob] panel each; bf16x3 engine:
 *   fwd:   y[r][k*ob + o]  = act(sum_i x[r][k*ib + i] * w[k][i][o])
 *   dgrad: gx[r][k*ib + i] = (sum_o gy[r][k*ob + o] * conj(w[k][i][o])) * mask(a[r][k*ib + i])
 *   wgrad: gw[k][i][o]     = sum_r conj(x[r][k*ib + i]) * gy[r][k*ob + o]
 *   mask:  out[e]          = s[e] != 0 ? gy[e] : 0          over n floats (components), out may alias gy
 * w: complex [nb][ib][ob] (view_as_complex of the reference's [nb, ib, ob, 2] parameter).  act: 0 none, 2 ReLU on both
 * components, 3 soft-shrink with threshold lambda >= 0 on both components (v > lambda: v - lambda, v < -lambda: v + lambda, else
 * +0), applied in fp32 on the accumulator.  a: the saved activation OUTPUT of the layer in front ([rows][nb*ib], act = 2: a
 * component passes where the same component of a is > 0) or NULL with act = 0.  There is no bias.
 * softshrink' is read off the saved soft-shrink OUTPUT s by the pointwise `mask` pass (one read of gy and s, one write), whose
 * result is the gy of both dgrad and wgrad of that layer.
 * The weight gradient contracts groups of rows into partial panels in `workspace` (mk_spec_bdmlp_wgrad_workspace bytes, 16-byte
 * aligned; 0 bytes: not needed) and adds them in ascending order: no atomics, the same bits on every run.
 * ib, ob even (block offsets stay 16-byte aligned), operands 16-byte aligned, 129 rows of a field and one panel below 2^31 bytes. */
int mk_spec_bdmlp_fwd(const float* x, const float* w, float* y, int rows, int nb, int ib, int ob, int act, float lambda,
                      void* stream);
int mk_spec_bdmlp_dgrad(const float* gy, const float* w, const float* a, float* gx, int rows, int nb, int ib, int ob, int act,
                        void* stream);
long long mk_spec_bdmlp_wgrad_workspace(int rows, int nb, int ib, int ob);
int mk_spec_bdmlp_wgrad(const float* x, const float* gy, float* gw, void* workspace, int rows, int nb, int ib, int ob,
                        void* stream);
int mk_spec_bdmlp_mask(const float* gy, const float* s, float* out, long long n, void* stream);
/* The forward product with a complex bias per output channel, the spectral MLP of the channels-last AFNO
 * (networks/afnonet.py:81-103: `relu(x w1 + b1)`, then `x w2 + b2` in front of the soft-shrink of line 106):
 *   y[r][k*ob + o] = act(sum_i x[r][k*ib + i] * w[k][i][o] + bias[k*ob + o])
 * bias: interleaved complex [nb * ob], 8-byte aligned, added in fp32 on the accumulator before act (0, 2 or 3 as above); NULL is
 * mk_spec_bdmlp_fwd, bit for bit.  The data and weight gradients are those of the family above; the bias gradient is
 * mk_spec_cmlp_bgrad of the (masked) output gradient with cout = nb * ob on a dense spectrum. */
int mk_spec_bdmlp_fwd_bias(const float* x, const float* w, const float* bias, float* y, int rows, int nb, int ib, int ob, int act,
                           float lambda, void* stream);

/* ---- "diagonal" spectral filter: one complex weight per (l, m) ---------------------------
 * Public layout, P = L * M contiguous: x [B][I][P], w [I][O][P], y [B][O][P] complex64.
 *   y[b][o][p] = sum_i x[b][i][p] * w[i][o][p]
 * Replaces _contract_diagonal `einsum("bixy,ioxy->boxy")` (contractions.py:121-127) and its gradients
 *   gx[b][i][p] = sum_o gy[b][o][p] * conj(w[i][o][p]),   gw[i][o][p] = sum_b conj(x[b][i][p]) * gy[b][o][p].
 * Elementwise in p (1 flop per weight byte): HBM-streaming kernels, exact fp32 fma chains. */
int mk_diag_fwd(const float* x, const float* w, float* y, int batch, int cin, int cout, long long P, void* stream);
int mk_diag_dgrad(const float* gy, const float* w, float* gx, int batch, int cin, int cout, long long P, void* stream);
int mk_diag_wgrad(const float* x, const float* gy, float* gw, int batch, int cin, int cout, long long P, void* stream);

/* ---- diagonal spectral filter on the private spectrum -------------------------------------------
 * The same contraction without the layout round trip: x / y / gx / gy are the private spectrum [lloc][mloc][batch * chan]
 * complex64 (channel contiguous, as for dhconv), w / gw the parameter as stored, [cin][cout][lloc][mloc] complex64.
 * dense = 0: entries with global l_off + l < m_off + m hold no data -- x / gy / w there are never read, y / gx there are not
 * written, gw there is an exact zero written by the kernel.  dense = 1 (the planar pair): every entry is data.
 * Exact sequential fp32 fma chains in the order of mk_diag_*; one writer per element: the same bits every run and for every
 * cut into shards.  Operands 8-byte aligned (16-byte weight accesses where mloc is even and w is 16-byte aligned);
 * cin + cout <= 2500, batch <= 65536. */
/* y[l][m][b][o] = sum_i x[l][m][b][i] * w[i][o][l][m]   (_contract_diagonal, contractions.py:121-127) */
int mk_spec_diag_fwd(const float* x, const float* w, float* y, int lloc, int mloc, int batch,
                     int cin, int cout, int l_off, int m_off, int dense, void* stream);
/* gx[l][m][b][i] = sum_o gy[l][m][b][o] * conj(w[i][o][l][m])   (adjoint in x of contractions.py:121-127) */
int mk_spec_diag_dgrad(const float* gy, const float* w, float* gx, int lloc, int mloc, int batch,
                       int cin, int cout, int l_off, int m_off, int dense, void* stream);
/* gw[i][o][l][m] = sum_b conj(x[l][m][b][i]) * gy[l][m][b][o]   (adjoint in w of contractions.py:121-127) */
int mk_spec_diag_wgrad(const float* x, const float* gy, float* gw, int lloc, int mloc, int batch,
                       int cin, int cout, int l_off, int m_off, int dense, void* stream);

/* ---- layout conversion -------------------------------------------------- */
/* torch [BC][L][M] complex64  <->  private [L][M][BC] complex64.  unpack writes
 * exact zeros where global l < m (what the reference's zero table entries give). */
int mk_spec_pack(const float* c_std, float* c_prv, int bc, int lloc, int mloc, void* stream);
int mk_spec_unpack(const float* c_prv, float* c_std, int bc, int lloc, int mloc,
                   int l_off, int m_off, void* stream);
/* tokens [batch][n][c]  <->  fields [batch][c][n]: what lets the channels-last AFNO (networks/afnonet.py:63-112, `rfft2(x,
 * dim=(1, 2))` on x [B, H, W, C], n = H * W) run on the planar transforms, which read channel-major fields.
 *   tokens_to_fields: fld[b][ch][i] = tok[b][i][ch]
 *   fields_to_tokens: tok[b][i][ch] = fld[b][ch][i] + addend[b][i][ch]     (addend NULL: the plain transpose)
 * The addend is the filter's `x + bias` (afnonet.py:112) in the pass that brings the inverse transform's rows back to tokens.
 * dtype: 0 fp32, 1 bf16, the same on all operands; the add is in fp32, rounded once.  Any batch, n, c >= 1 (64-bit offsets);
 * 16-byte loads and stores where n, c are multiples of 16 bytes' worth of elements and the operands 16-byte aligned, single
 * elements otherwise.  One launch, no allocation, no synchronisation.  Each is the adjoint of the other. */
int mk_tokens_to_fields(const void* tok, void* fld, int dtype, int batch, int n, int c, void* stream);
int mk_fields_to_tokens(const void* fld, const void* addend, void* tok, int dtype, int batch, int n, int c, void* stream);
/* image [batch][C][H][W]  <->  patch rows [batch hp wp][ldt] (csrc/patch.hip): the gather in front of the patch-embedding GEMM of
 * ViT / AFNOv1 (a non-overlapping strided convolution is one GEMM on these rows) and the un-patchify behind their heads.
 * hp = H / p0, wp = W / p1; row r = (b hp + y) wp + x holds the patch at (y p0, x p1); element (b, c, y p0 + i, x p1 + j) is feature
 *   order 0: f = (c p0 + i) p1 + j      the order of a convolution weight [E][C][p0][p1] seen as [E][C p0 p1]
 *   order 1: f = (i p1 + j) C + c       the order both heads write (`einsum("nhwpqc->nchpwq")`, `permute(0, 5, 1, 3, 2, 4)`)
 *   mk_patchify:   tok[r][f] = img[b][c][y p0 + i][x p1 + j]
 *   mk_unpatchify: the inverse; for one order each is the other's inverse and adjoint.
 * dtypes: 0 fp32, 1 bf16 on either side, in every combination: narrowing rounds once to nearest even (a NaN becomes 0x7fc0),
 * widening is exact, equal dtypes pass bit for bit.  ldt >= C p0 p1 is the row stride in elements; columns past C p0 p1 are
 * neither read nor written.  Any batch, C, p0, p1 >= 1 and H, W the patch divides; bases aligned to their elements; 64-bit
 * offsets.  16-byte loads and stores on a side whose base is 16-byte aligned and whose contiguous runs are whole vectors, single
 * elements otherwise; both sides walk their contiguous axis (a tile goes through LDS).  Every destination element is written
 * exactly once.  One launch, no allocation, no synchronisation; arguments are validated (code 1) before the launch. */
/* The tile the two kernels use for a geometry (no device needed): tile[14] = CC channels, IT patch rows, TX patches across, JT
 * patch columns, the LDS row pitch in words, the tile counts along channels / patch rows / patches across / patch columns, the
 * words of LDS a workgroup has, and whether 16-byte-aligned bases would take 16-byte accesses on the image side (fp32, bf16)
 * and on the token side (fp32, bf16) at row stride ldt.  tests/test_patch_cpu.py runs a model of the index maps on it. */
int mk_patch_tile_info(int C, int H, int W, int p0, int p1, int order, long long ldt, int* tile);
int mk_patchify(const void* img, int img_dtype, void* tok, int tok_dtype, long long ldt, int batch, int C, int H, int W, int p0,
                int p1, int order, void* stream);
int mk_unpatchify(const void* tok, int tok_dtype, long long ldt, void* img, int img_dtype, int batch, int C, int H, int W, int p0,
                  int p1, int order, void* stream);

/* ---- fused pointwise ops of the FNO block (rows = B*C <= 65535, P = H*W multiple of 8) -------- */
/* dtype: 0 = fp32, 1 = bf16 storage; arithmetic is fp32.
 * y = gelu(x + bias[row % C]) (exact erf GELU).  Replaces the bias add of nn.Conv2d(.., 1) followed by
 * nn.GELU in MLP / EncoderDecoder (makani/models/common/layers.py:95-99,158-206). */
int mk_bias_gelu_fwd(const void* x, const float* bias, void* y, int dtype, int rows, int C, long long P,
                     void* stream);
/* gx = gy * gelu'(x + bias); gbias[c] += sum over (b, p) of gx (caller zeroes gbias; may be NULL). */
int mk_bias_gelu_bwd(const void* x, const float* bias, const void* gy, void* gx, float* gbias, int dtype,
                     int rows, int C, long long P, void* stream);
/* y = r + affine[row][0] * z + affine[row][1]: the apply pass of an instance norm (coefficients from mk_instnorm_coeffs)
 * with the skip add, for a skip that was synthesised from the spectrum (mk_spec_mix_fwd).  affine fp32 [rows][2]. */
int mk_affine_add(const void* r, const void* z, const float* affine, void* y, int dtype, int rows, long long P,
                  void* stream);
/* Instance norm over each row, y = act(((x - mean) * rstd) * weight[c] + bias[c]), biased variance,
 * act = GELU if fuse_gelu else identity.  stats[row] = (mean, rstd) is kept for the backward;
 * workspace: 2*rows doubles (zeroed inside).  Replaces nn.InstanceNorm2d(eps=1e-6, affine=True)
 * (+ act_layer0) of FourierNeuralOperatorBlock (makani/models/networks/sfnonet.py:239-253,375-380). */
int mk_instnorm_fwd(const void* x, const float* weight, const float* bias, void* y, float* stats,
                    double* workspace, int dtype, int rows, int C, long long P, float eps, int fuse_gelu,
                    void* stream);
/* gx of the above; on return workspace[row] = (sum g', sum g' * xhat) with g' = gy * act'(z), from which
 * the caller forms gbias[c] = sum_b workspace[b, c, 0], gweight[c] = sum_b workspace[b, c, 1]. */
int mk_instnorm_bwd(const void* x, const void* gy, const float* stats, const float* weight, const float* bias,
                    void* gx, double* workspace, int dtype, int rows, int C, long long P, int fuse_gelu,
                    void* stream);

/* Split-phase forms for rows sharded over ranks (DistributedInstanceNorm2d, makani/mpu/layer_norm.py:27-114):
 * phase 1 = local row sums into `workspace` ([rows][2] doubles: sum x, sum x^2 / sum g', sum g' xhat);
 * the caller all-reduces `workspace` over the ranks sharing the rows; phase 2 = apply with the reduced sums and
 * `count` = the global number of elements per row.  phase 0 = both (count = P): the single-GPU calls above. */
int mk_instnorm_fwd_ex(const void* x, const float* weight, const float* bias, void* y, float* stats,
                       double* workspace, int dtype, int rows, int C, long long P, long long count, float eps,
                       int fuse_gelu, int phase, void* stream);
int mk_instnorm_bwd_ex(const void* x, const void* gy, const float* stats, const float* weight, const float* bias,
                       void* gx, double* workspace, int dtype, int rows, int C, long long P, long long count,
                       int fuse_gelu, int phase, void* stream);
/* mk_instnorm_bwd for one sample (rows = C) that also writes the gradients of the affine parameters: gwb fp32 [2][C], row 0 =
 * weight gradient (sum g' xhat), row 1 = bias gradient (sum g'), the backward of `nn.InstanceNorm2d(affine=True)`'s parameters
 * (sfnonet.py:239-253) without a copy / cast launch behind the kernel. */
int mk_instnorm_bwd_wb(const void* x, const void* gy, const float* stats, const float* weight, const float* bias, void* gx,
                       double* workspace, float* gwb, int dtype, int C, long long P, int fuse_gelu, void* stream);

/* ---- 1x1 convolution weight gradient (bf16 MFMA) ------------------------------------------ */
/* Latitude-weighted squared error of the training harness (latitude weights as in
 * makani/utils/losses.py:149-271):  loss = scale * sum_{r,w} wrow[r % H] * (pred[r][w] - tar[r][w])^2 over rows
 * r = (b, c, h) of W points (W % 8 == 0); pred fp32 (dtype 0) or bf16 (1), tar fp32, loss one double (zeroed here).
 * Backward: gpred = 2 * scale * gloss[0] * wrow[r % H] * (pred - tar) in pred's dtype. */
int mk_wmse_fwd(const void* pred, int dtype, const float* tar, const float* wrow, double* loss, long long rows,
                int H, int W, float scale, void* stream);
int mk_wmse_bwd(const void* pred, int dtype, const float* tar, const float* wrow, const float* gloss, void* gpred,
                long long rows, int H, int W, float scale, void* stream);

/* The same convolutions on fp32 fields (no autocast), fp32-accurate on the bf16x3 engine of the spectral GEMMs (csrc/gemm_x3.hip):
 *   mode 0:  c[b] = a b[b]            a [M][K] row-major (lda a multiple of 4, rows zero-padded to K rounded up to 4), b[b] [K][N] = the NCHW field (N = H*W even)
 *   mode 1:  c[b] += a b[b]           (a skip connection folded into the GEMM: c holds the addend)
 *   mode 2:  c += sum_b a[b] b[b]^T   a[b] [M][K], b[b] [N][K], K = H*W the contraction: the weight gradient (c zeroed by the caller, fp32 atomics)
 * sa / sb / sc = batch strides in elements.  Replaces F.conv2d / its gradients behind nn.Conv2d(.., 1) in fp32 mode (layers.py:95-206). */
int mk_conv1x1_x3(const float* a, long long lda, const float* b, long long ldb, float* c, long long ldc, int M, int K, long long N,
                  int batch, long long sa, long long sb, long long sc, int mode, void* stream);
/* c[b] = act(a b[b] + bias): mode 0 with the bias add (bias fp32 [M] or NULL) and, with act = 1, the exact (erf) GELU in the epilogue:
 * `nn.Conv2d(cin, cout, 1, bias=True)` followed by `nn.GELU()` (layers.py:95-99, 158-206) in one pass over the output. */
int mk_conv1x1_x3_bias_act(const float* a, long long lda, const float* b, long long ldb, float* c, long long ldc, int M, int K,
                           long long N, int batch, long long sb, long long sc, const float* bias, int act, void* stream);

/* gw[o][i] += sum over (b, p) of gy[b][o][p] * x[b][i][p]; gy, x bf16 [B][C][P] (P multiple of 8), gw fp32
 * [cout][cin] accumulated with atomics (caller zeroes it).  The weight gradient of nn.Conv2d(cin, cout, 1)
 * in MLP / EncoderDecoder / skip connections (layers.py:95-128,158-183; sfnonet.py:207,463). */
int mk_conv1x1_wgrad(const void* gy, const void* x, float* gw, int batch, int cout, int cin, long long P,
                     void* stream);
/* The same with an activation applied to x while it is staged: x_act = 1 multiplies with GELU(x) (exact erf form,
 * rounded to bf16).  The weight gradient of the SECOND convolution of an MLP (layers.py:158-206) from the kept
 * pre-activation: with mk_pce_mlp the activated hidden field is never written.  cout <= 384. */
int mk_conv1x1_wgrad_act(const void* gy, const void* x, float* gw, int batch, int cout, int cin, long long P, int x_act,
                         void* stream);
/* Pixel-column engine (csrc/pce.hip): the same 1x1 convolutions as one persistent kernel per GEMM with the
 * pointwise passes of layers.py:86-216 / sfnonet.py:239-267 folded into the epilogue:
 *   acc[b][m][p] = sum_k A[m][k] * x[b][k][p] (+ bias[m]);   aux_out <- acc (bf16, optional: the pre-activation kept for
 *   the backward pass);   v = gelu ? GELU(acc) : acc;   v *= GELU'(aux_in[b][m][p]) (optional: backward of the activation);
 *   y = v (+ addend[b][m][p]).
 * A comes pre-packed (mk_pce_pack) as the MFMA fragment image of W [M][K] (forward) or of W^T (data gradient).
 * x, y, addend, aux_* are bf16 [B][C][P], P a multiple of 8; K <= 768, M <= 1536; bias is fp32 [M]
 * (or NULL); addend and aux_in are exclusive.
 * Replaces hipBLASLt's mm/addmm behind nn.Conv2d(.., 1) and the separate bias+GELU passes. */
long long mk_pce_image_bytes(int M, int K);
int mk_pce_pack(const void* w, int w_dtype /* 0 fp32, 1 bf16 */, int transpose, int M, int K, int ldw, void* img,
                void* stream);
/* All weight images of a net in ONE launch: desc_dev = n descriptors of 10 x int64 {weight pointer, dtype (0 fp32 / 1 bf16),
 * transpose, M, K, leading dimension, TH, steps per pass, core elements (the last three from mk_pce_pack_layout), first element in
 * the arena}, sorted by first element; image e occupies mk_pce_image_bytes(M, K) bytes from arena + 2 * first (the 64 zero bytes
 * included).  Replaces the per-call mk_pce_pack of every 1x1 convolution of a training step (56 launches at the SFNO config). */
int mk_pce_pack_layout(int M, int K, long long* out3);
int mk_pce_pack_batch(const void* desc_dev, int n, void* arena, long long total_elements, void* stream);
int mk_pce_gemm(const void* x, const void* wimg, void* y, const float* bias, const void* addend, const void* aux_in,
                void* aux_out, int gelu, int batch, int M, int K, long long P, void* stream);
/* The same with two more seams to the instance norms around the convolutions (sfnonet.py:262-267):
 *  - rowstats [B][M][2] (double, zeroed by the call; M <= 768) receives sum and sum of squares over the pixels of every
 *    stored y row: the statistics pass of the norm that follows an MLP, and the bias gradient of a convolution (sum over
 *    pixels of the output gradient), without another pass over the field;
 *  - addend_affine [B][M][2] (float) makes the addend enter as a * addend + b per row: the APPLY pass of the instance norm
 *    in front of a skip connection (coefficients from mk_instnorm_coeffs), folded into the skip convolution. */
int mk_pce_gemm_ex(const void* x, const void* wimg, void* y, const float* bias, const void* addend, const float* addend_affine,
                   const void* aux_in, void* aux_out, int gelu, double* rowstats, int batch, int M, int K, long long P,
                   void* stream);
/* Fused two-layer node (csrc/pce_mlp.hip): conv1x1 -> GELU -> conv1x1 of `MLP` / `EncoderDecoder` (layers.py:86-216; call
 * sites sfnonet.py:207,379,463) as ONE launch with the Hd-row hidden field kept on chip:
 *   mode 0 (forward):   mid_out = A1 x + b1  (bf16 [B][Hd][P], the pre-activation kept for backward);
 *                       y = A2 GELU(mid_out) (+ b2);   rowstats_y as in mk_pce_gemm_ex (or NULL)
 *   mode 1 (backward):  mid_out = (A1 x) * GELU'(mid_in)  (x = the output gradient, mid_in = the kept pre-activation:
 *                       mid_out is the gradient w.r.t. the pre-activation, operand of the first weight gradient);
 *                       y = A2 mid_out (the input gradient);   rowsum_mid [B][Hd] (double, zeroed by the call, or NULL) receives
 *                       the pixel sums of mid_out = the gradient of b1
 * A1 [Hd][K1] and A2 [M][Hd] come packed by mk_pce_mlp_pack (forward: W1, W2; backward: W2^T, W1^T -- `*_transposed` says
 * the array holds the transpose, i.e. a1 is [K1][Hd] / a2 is [Hd][M]).  K1 <= 384, Hd <= 768, M <= 384; x, y, mid_* bf16,
 * P a multiple of 8, biases fp32 or NULL. */
long long mk_pce_mlp_image_bytes(int M, int Hd, int K1);
int mk_pce_mlp_pack(const void* a1, int a1_transposed, int lda1, const void* a2, int a2_transposed, int lda2,
                    int w_dtype /* 0 fp32, 1 bf16 */, int M, int Hd, int K1, void* img, void* stream);
int mk_pce_mlp(const void* x, const void* wimg, void* y, void* mid_out, const void* mid_in, const float* b1, const float* b2,
               double* rowstats_y, double* rowsum_mid, int mode, int batch, int M, int Hd, int K1, long long P, void* stream);
/* Profiling aid (tools/mlp_stamps.py; build with -DMK_MLP_STAMPS, MK_MLP_DBG=1): s_memtime stamps of workgroup 0, 4 x 128. */
int mk_pce_mlp_debug_stamps(unsigned long long* out512);
/* Per-row coefficients of an instance norm from its row sums: stats[row] = (mean, rstd) (the form mk_instnorm_bwd takes),
 * affine[row] = (rstd * weight[c], bias[c] - mean * rstd * weight[c]); count = elements per row (global, when sharded). */
int mk_instnorm_coeffs(const double* sums, const float* weight, const float* bias, float* stats, float* affine, int rows,
                       int C, long long count, float eps, void* stream);
/* Profiling aid (tools/pce_stamps.py): with MK_PCE_DBG=1 in the environment the kernel records s_memtime stamps of
 * workgroup 0; this copies the 8 x 64 stamps of the last launch to the host. */
int mk_pce_debug_stamps(unsigned long long* out512);

/* One Adam step (torch.optim.Adam semantics: L2 weight decay folded into the gradient, bias-corrected moments, no
 * amsgrad) over n contiguous fp32 elements in one streaming pass; `step` is the 1-based step count.  The optimizer
 * step of the training harness (makani/utils/trainer.py:762-763); complex parameters are stepped as 2 n reals. */
int mk_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int step, void* stream);

/* ---- multi-tensor optimizer kernels (optim.hip) ------------------------
 * The optimizers of the reference trainer's `optimizer_type` switch (makani/utils/trainer.py:448-478: torch AdamW /
 * Adam, apex FusedLAMB) and the gradient clipping of its `max_grad_norm`.  A tensor list is `T` fp32 runs given as
 * host arrays: device addresses (4-byte aligned; for the 4-stream calls p, g, m, v of tensor t at [4 t .. 4 t + 3])
 * and lengths in reals.  The list is passed by value to the kernels (captured launches upload nothing); lists longer
 * than one argument block take several launches.  Norm partials are fp64, one per chunk of a tensor: a workspace
 * `partials` holds sum over t of mk_mt_chunks(n[t]) doubles, `tsum` T doubles.  Deterministic: no float atomics.
 * Step counts: `steps` == NULL -> step_or_slot[t] is the (1-based) step of tensor t; else it is the slot of tensor t
 * in the float32 device table `steps` (capturable mode), whose slots `inc_slots` are incremented by the norm's
 * finalize (or by mk_mt_step_inc) before any update reads them.  `lr_dev` != NULL: the learning rate is read there. */
/* Norm partials a tensor of n reals produces. */
long long mk_mt_chunks(long long n);
/* Per-tensor sums of squares tsum[t] (torch.nn.utils.clip_grad_norm_, trainer.py:757-760; apex FusedLAMB's global
 * norm).  clip_mode 0: tsum only; 1: also the norm G and torch's coefficient min(1, max_norm / (G + 1e-6));
 * 2: G and apex LAMB's divisor (G > max_norm ? G / max_norm : 1); 3: G alone.  norm_out / coef_out: device floats. */
int mk_mt_sumsq(int T, const uint64_t* x, const long long* n, double* partials, double* tsum, int clip_mode, float max_norm,
                float* norm_out, float* coef_out, float* steps, const int* inc_slots, int ninc, void* stream);
/* The total and the coefficient from tsum (after tsum was summed over the model-parallel groups); same clip_mode. */
int mk_mt_norm_finish(int T, const double* tsum, int clip_mode, float max_norm, float* norm_out, float* coef_out,
                      float* steps, const int* inc_slots, int ninc, void* stream);
/* steps[slots[i]] += 1 (capturable step counter when no norm pass runs before the update). */
int mk_mt_step_inc(float* steps, const int* slots, int nslots, void* stream);
/* x *= *coef over every tensor (clip_grad_norm_'s in-place rescale). */
int mk_mt_scale(int T, const uint64_t* x, const long long* n, const float* coef, void* stream);
/* torch.optim.AdamW (adamw = 1: p *= 1 - lr wd) or torch.optim.Adam (adamw = 0: g += wd p) in one pass; the gradient
 * is multiplied by *coef as it is read (coef may be NULL) and is not written.  Bias corrections in double. */
int mk_mt_adam(int T, const uint64_t* pgmv, const long long* n, const int* step_or_slot, const float* steps, float lr,
               const float* lr_dev, float beta1, float beta2, float eps, float weight_decay, int adamw, const float* coef,
               void* stream);
/* apex FusedLAMB (apex/optimizers/fused_lamb.py, csrc/multi_tensor_lamb.cu), gradient divided by *coef (NULL: 1).
 * Stage 1 updates m, v and leaves the per-tensor sums of squares of the old p (tsum_p) and of the update u (tsum_u);
 * stage 2 recomputes u from the new moments and applies p -= r u, r = lr |p| / |u| when `trust` and both are non-zero,
 * else lr.  The gradient is not overwritten. */
int mk_mt_lamb(int stage, int T, const uint64_t* pgmv, const long long* n, const int* step_or_slot, const float* steps,
               float lr, const float* lr_dev, float beta1, float beta2, float beta3, float eps, float weight_decay, int adamw,
               int bias_correction, int trust, const float* coef, double* part_p, double* part_u, double* tsum_p,
               double* tsum_u, void* stream);

/* ---- validation metrics (csrc/metrics.hip): geometric L1, RMSE and ACC of the trainer's MetricsHandler
 * (makani/utils/metrics/functions.py:20-107, makani/utils/metric.py:186-204) as five latitude-weighted integrals per
 * (sample, channel), written to sums [B][C][5] (fp64) in the order
 *   sum w |p - t|,  sum w (p - t)^2,  sum w (p - c)(t - c),  sum w (p - c)^2,  sum w (t - c)^2
 * with w = wrow[h] and c = clim[c][h][w] (c = 0 when clim is NULL).  pred [B][C][H][W] fp32 (dtype 0) or bf16 (1),
 * tar [B][C][H][W] fp32, clim [C][H][W] fp32 shared by all samples, wrow [H] fp32; any W and any element-aligned
 * pointers.  The sums add up over spatial shards (the caller slices wrow and clim to its shard).  Deterministic (no
 * atomics); no allocation, synchronisation or host copy: `workspace` holds mk_geo_metric_workspace(B, C, H) doubles. */
long long mk_geo_metric_workspace(int B, int C, int H);
int mk_geo_metric_sums(const void* pred, int dtype, const float* tar, const float* clim, const float* wrow, double* workspace,
                       double* sums, int B, int C, int H, int W, void* stream);

/* ---- training losses of the Lp family (csrc/lploss.hip): every spelling of GeometricLpLoss
 * (makani/utils/losses.py:174-271) is a function of two latitude-weighted integrals per (sample, channel), written to
 * sums [B][C][2] (fp64) in the order
 *   s0 = sum w |p - t|^P,   s1 = sum w |t|^P,   P = p in {1, 2},   w = wrow[h].
 * pred [B][C][H][W] fp32 (dtype 0) or bf16 (1), tar [B][C][H][W] fp32, wrow [H] fp32; any W and any element-aligned
 * pointers.  The sums add up over spatial shards (the caller slices wrow to its shard).  Deterministic (no atomics); no
 * allocation, synchronisation or host copy: `workspace` holds mk_geo_lp_workspace(B, C, H) doubles.
 * Backward of s0 with respect to pred, g [B][C] fp32 on the device (the upstream gradient of s0):
 *   gpred = g[b][c] * wrow[h] * (p == 2 ? 2 (pred - tar) : sign(pred - tar)),  sign(0) = 0,  in pred's dtype. */
long long mk_geo_lp_workspace(int B, int C, int H);
int mk_geo_lp_sums(const void* pred, int dtype, const float* tar, const float* wrow, double* workspace, double* sums, int p,
                   int B, int C, int H, int W, void* stream);
int mk_geo_lp_bwd(const void* pred, int dtype, const float* tar, const float* wrow, const float* g, void* gpred, int p,
                  int B, int C, int H, int W, void* stream);

/* ---- input assembly of the step wrappers (csrc/preproc.hip): what makani/models/stepper.py builds before every model
 * call, add_static_features(history_normalize(append_unpredicted_features(x))), in one pass that reads every source
 * once and writes every output element once.
 *   x    [B][T][C][H][W]   predicted channels, T = n_history + 1, fp32 (dtype 0) or bf16 (1)
 *   u    [B][T][Cu][H][W]  unpredicted channels, fp32 (NULL exactly when Cu == 0)
 *   stat [Cs][H][W]        static features, fp32, shared by all samples (NULL exactly when Cs == 0)
 *   mean, std [B][C + Cu]  fp32, both or neither; given: v -> (v - mean) / std with a correctly rounded division
 *   mask_chans [n_mask]    int32 on the device: output channels (< T (C + Cu)) multiplied by stat[mask_src] pointwise
 *                          (entries outside that range match no row); mask_src is checked on the host
 *   out  [B][T (C + Cu) + Cs][H][W], channel t (C + Cu) + j = step t, channel j of (x | u); fp32 (0) or bf16 (1, RNE)
 * Any W and any element-aligned pointers.  No allocation, synchronisation or host copy.
 * Backward, the gradient of x only (statistics are constants):
 *   gx[b][t][c] = (gout[b][t (C + Cu) + c] * mask) / std[b][c]   (std NULL: no division), gout fp32 / bf16, gx in
 *   x's dtype. */
int mk_input_assemble(const void* x, int x_dtype, const float* u, const float* stat, const float* mean, const float* std,
                      const int* mask_chans, int n_mask, int mask_src, void* out, int out_dtype, int B, int T, int C, int Cu,
                      int Cs, int H, int W, void* stream);
int mk_input_assemble_bwd(const void* gout, int g_dtype, const float* stat, const float* std, const int* mask_chans, int n_mask,
                          int mask_src, void* gx, int x_dtype, int B, int T, int C, int Cu, int Cs, int H, int W, void* stream);

/* History statistics of Preprocessor2D.history_compute_stats as raw sums: sums [B][C + Cu][2] (fp64),
 *   sum_t wt[t] sum_hw v,   sum_t wt[t] sum_hw v^2,   v = (x | u)[b][t][j][h][w],   wt [T] fp32 on the device.
 * Accumulated in fp64 throughout, deterministic (no atomics); the sums add up over spatial shards.  No allocation,
 * synchronisation or host copy: `workspace` holds mk_history_workspace(B, C + Cu, H) doubles. */
long long mk_history_workspace(int B, int Cn, int H);
int mk_history_sums(const void* x, int x_dtype, const float* u, const float* wt, double* workspace, double* sums, int B, int T,
                    int C, int Cu, int H, int W, void* stream);

/* ---- the tail of an autoregressive rollout step (csrc/rollout.hip): everything makani/utils/inferencer.py and the step
 * wrappers do behind the model call, in one pass over the model output.  Every optional part is switched off by a NULL
 * pointer or a zero count.  Per point (b, c, h, w), in this order, every product and sum an fp32 rounding of its own (the
 * file is compiled with fp contraction off):
 *   v = yn[b][c][h][w]                           fp32 (dtype 0) or bf16 (1, widened exactly)
 *   v = v * std[b][c] + mean[b][c]               mean, std [B][C] fp32, both or neither
 *   v = v * mask[h][w]                           for c in mask_chans [n_mask] (int32, device); mask [H][W] fp32
 *   v = x_last[b][c][h][w] + v * scale[c]        when residual == 1; scale [C] fp32 or NULL (v = x_last + v);
 *                                                x_last fp32, sample b at x_last + b * x_bstride (elements), [C][H][W] there
 *   v = x_last[b][c][h][w]                       for c in hold_chans [n_hold] (int32, device)
 *   pred[b][c][h][w] = v                         fp32, each element written once
 *   with tar [B][C][H][W] fp32:  d = v - tar (rounded to fp32);  sums [B][C][6] fp64 = the five sums of mk_geo_metric_sums
 *     in its order (w = wrow[h], c = clim[c][h][w] or 0 when clim is NULL) and the unweighted sum d d;
 *     err_map [C][H][W] fp32 (or NULL) = (..((err_map + d_0 d_0) + d_1 d_1) ..) over the samples in ascending b
 *   emit[b][k][h][w] = v(c = emit_chans[k]) * emit_scale[k] + emit_shift[k],  k < K; emit_scale / emit_shift [K] fp32 or
 *     NULL (the product / the sum is then not formed: the value is copied); an entry of emit_chans outside [0, C) leaves
 *     its field unwritten, as an entry of mask_chans or hold_chans outside it matches no channel
 * clim, err_map and sums need tar; tar needs wrow, workspace (mk_rollout_tail_workspace(B, C, H) doubles) and sums.
 * pred, err_map and emit depend on their own point only: a launch on a slice of rows gives the slice bit for bit.  The
 * sums are accumulated as in mk_geo_metric_sums (fp32 row partials, fp64 across rows, slabs added in a fixed order): no
 * atomics, the same bits every run.  Any W and any element-aligned pointers.  No allocation, synchronisation or host
 * copy. */
long long mk_rollout_tail_workspace(int B, int C, int H);
int mk_rollout_tail(const void* yn, int dtype, const float* mean, const float* std, const float* mask, const int* mask_chans,
                    int n_mask, const float* x_last, long long x_bstride, int residual, const float* scale,
                    const int* hold_chans, int n_hold, float* pred, const float* tar, const float* clim, const float* wrow,
                    double* workspace, double* sums, float* err_map, float* emit, const int* emit_chans, const float* emit_scale,
                    const float* emit_shift, int K, int B, int C, int H, int W, void* stream);

/* ---- dataset statistics (csrc/stats.hip): what data_process/get_stats.py derives its seven files from, in one pass
 * over a batch x [T][C][H][W] of fp32 samples that are consecutive in time.  Every optional part is switched off by a
 * NULL pointer or a zero count.  Per channel c, with d = x - pivot[c] (pivot [C] fp32; NULL: 0), e = x_t - x_{t-1}, both
 * formed in fp64, and w = wrow[h] (wrow [H] fp32):
 *   sums [C][4] fp64   = sum w d,  sum w d^2,  sum w e,  sum w e^2          written, not accumulated
 *     e runs over t = 1 ... T-1, and over t = 0 too when prev [C][H][W] fp32 is given (the sample before the first);
 *     with T = 1 and no prev the two difference sums are exact zeros
 *   minmax [C][2] fp32 = min, max over the call; a NaN anywhere in a channel makes its min, max and four sums NaN
 *   tsum [C][H][W] fp64, read-modify-write:  tsum = (..((tsum + x_0) + x_1) ..) in ascending t, one thread per point:
 *     bit-equal to a sequential fp64 sum, and a launch on a slice of rows gives that slice bit for bit
 *   wsums [n_wind][2] fp64 = sum m,  sum m^2 (unweighted) for the pairs (wind_u[k], wind_v[k]) (int32, device),
 *     m = sqrtf(u u + v v) in fp32: each product rounded, the sum rounded, the root correctly rounded (no fma), then
 *     widened.  The u channels must differ: a pair whose u repeats an earlier pair's, or with an index outside [0, C),
 *     reads nothing and gets NaN sums.  The v channel of a pair is read a second time.
 * All accumulation is fp64 (a lane adds the unweighted terms of a row and folds them with the row's weight at its end);
 * every workgroup writes a workspace slot of its own and a finish adds the slots in a fixed order: no atomics, the same
 * bits every run.  The sums add up over spatial shards and over calls with one pivot (the caller slices wrow to its
 * shard).  Element offsets are 64-bit (T C H W may pass 2^31); C <= 65535 and C H W < 2^31.  Any W and any
 * element-aligned pointers.  No allocation, synchronisation or host copy: `workspace` holds
 * mk_field_stats_workspace(C, H, n_wind) doubles. */
long long mk_field_stats_workspace(int C, int H, int n_wind);
int mk_field_stats(const float* x, const float* prev, const float* pivot, const float* wrow, double* workspace, double* sums,
                   float* minmax, double* tsum, const int* wind_u, const int* wind_v, int n_wind, double* wsums, int T, int C,
                   int H, int W, void* stream);

/* ---- dataset histograms (csrc/hist.hip): the second sweep of data_process/get_histograms.py, np.histogram per channel
 * over a given range, in one pass over a batch x [T][C][H][W] of fp32 samples.
 *   edges [C][nbins + 1] fp64: per channel a strictly increasing table (an fp32 table is widened by the caller, which
 *     is exact).  Whether it increases cannot be checked through a device pointer: that is the caller's check
 *   counts [C][nbins] int64, ADDED TO: the caller zeroes it once and batches accumulate.  The counts are the ones the
 *     table defines, exactly: bin i holds edges[i] <= x < edges[i + 1], the last bin is closed on the right.  The bin of
 *     a point is guessed by fp32 arithmetic and corrected against the table, so no rounding of the guess reaches a count
 *   outside [C][3] int64, added to, or NULL: the points below edges[0] (-inf among them), above edges[nbins] (+inf) and
 *     the NaNs, none of which is binned (np.histogram drops them silently)
 * Workgroup (slab of 4 rows, channel) keeps the channel's table, as the exact fp32 thresholds up(edges[i]) (x >= e for
 * an fp32 x is x >= the smallest fp32 not below e), and R replicas of a uint32 bin array in LDS (lane -> replica, runs
 * of equal bins among a lane's 8 points merged into one add), folds the replicas and adds its non-zero bins
 * to counts with device-scope 64-bit INTEGER atomics: integer addition commutes and does not round, so the result is
 * the same every run and for every split of the rows or the samples -- which is why atomics are acceptable here, where
 * the floating-point sums of this library avoid them.  nbins is 1 ... 4096: the table and one bin array then take 32,776
 * bytes of LDS (plus 48 static) and four workgroups fit a CU of 160 KB; more bins would run on fewer.  C <= 65535, C H W < 2^31, and 4 W T < 2^32 (a
 * workgroup's points fit a uint32 bin); element offsets are 64-bit.  Any W; x at any 4-byte aligned address, every
 * (sample, row) vectorised from its own 16-byte boundary; edges, counts and outside 8-byte aligned.  Every refusal
 * returns 1 before any launch.  No workspace, one launch, no allocation, synchronisation or host copy. */
int mk_field_hist(const float* x, const double* edges, long long* counts, long long* outside, int nbins, int T, int C, int H,
                  int W, void* stream);

/* ---- ensemble scores (csrc/ens.hip): CRPS, spread, ensemble-mean error and the rank histogram of an ensemble
 * ens [B][E][C][H][W] (fp32: dtype 0, bf16: 1) against a target tar [B][C][H][W] fp32, in one pass.  A member's [C][H][W]
 * block is contiguous; bstride and estride are the batch and member strides in ELEMENTS (a [B E][C][H][W] model output is
 * read in place with bstride = E C H W, estride = C H W; larger strides leave gaps that are never read).  Per point, with
 * the members x_e and the target y widened to fp64 and every value formed in fp64:
 *   a = (1/E) sum_e |x_e - y|
 *   g = (1/E^2) sum_e sum_f |x_e - x_f|, computed as (2/E^2) sum_k (2k - E - 1) x_(k) over the members sorted ascending
 *   m = (1/E) sum_e x_e,  q = (m - y)^2,  v = (1/(E - 1)) sum_e (x_e - m)^2 (two-pass about m)
 *   r = #{e : x_e < y}: a tie with the target counts as not less
 *   sums [B][C][4] fp64 = sum_hw wrow[h] (a, g, q, v), wrow [H] fp32          written, not accumulated
 *     CRPS = a - g / 2, fair CRPS = a - g E / (2 (E - 1)), spread^2 = v, squared error of the ensemble mean = q
 *   ranks [C][E + 1] int64, ADDED TO, or NULL: the histogram of r over b, h, w
 *   skipped [C] int64, added to, or NULL: the points whose target or one of whose members is NaN.  Such a point is not
 *     ranked and makes all four sums of its (b, c) NaN (the sorting network alone would drop the NaN: it is looked for
 *     before the sort).  Infinite inputs are out of contract
 * E is 2 ... 64: a thread sorts the E fp32 members of its point (ordering fp32 values loses nothing) in P registers, P the
 * power of two >= E, padded with +inf that the rank weights never touch.  Workgroup (slab of 8 rows, channel, sample)
 * stages tiles of 256 (P = 64: 128) consecutive points through LDS, every member and the target from its OWN 16-byte
 * boundary (scalar head, 16-byte body, scalar tail): any W, any element-aligned pointers and strides.  Sums are
 * accumulated in fp64 per thread, folded in a fixed order and written to a workspace slot per workgroup; a finish adds
 * the slabs in slab order: no floating-point atomics, the same bits every run.  Ranks and skipped go through LDS to
 * device-scope 64-bit INTEGER atomics, which commute and do not round: the same counts every run and for every split
 * of the rows.  Element offsets are 64-bit (B E C H W may pass 2^31); B, C <= 65535.  The file is compiled with fp
 * contraction off.  Every refusal returns 1 before any launch.  Two launches, no allocation, synchronisation or host
 * copy: `workspace` holds mk_ens_workspace(B, C, H) doubles. */
long long mk_ens_workspace(int B, int C, int H);
int mk_ens_sums(const void* ens, int dtype, long long bstride, long long estride, const float* tar, const float* wrow,
                double* workspace, double* sums, long long* ranks, long long* skipped, int B, int E, int C, int H, int W,
                void* stream);

/* The gradient of the first two sums, S [B][C][2] = sum_hw wrow[h] (a, g), with respect to the members: the backward of the
 * ensemble CRPS loss a - (kappa / 2) g (kappa = 1: CRPS, kappa = E / (E - 1): fair CRPS).  With the upstream gradient
 * gs [B][C][2] fp64, L_e = #{f : x_f < x_e} and G_e = #{f : x_f > x_e},
 *   gens[b][e][c][h][w] = wrow[h] (gs[b][c][0] sgn(x_e - y) / E + gs[b][c][1] 2 (L_e - G_e) / E^2),   sgn(0) = 0
 * which is what autograd gives for the all-pairs expression (abs'(0) = 0): tied members get the same value and the member
 * order does not matter (the gradient through a sort hands tied members different values).  If the target or any member
 * of a point is NaN, the gradient of EVERY member of that point is NaN.  No gradient goes to the target.
 * The comparisons are fp32 (exact: members are fp32, or bf16 widened), the counts integers; wrow, gs[.][.][0] / E and
 * 2 gs[.][.][1] / E^2 are fp64, the value is formed in fp64 and rounded ONCE to the gradient's dtype, which is the
 * members' (a bf16 value is not rounded through fp32).  E is 2 ... 16: a thread holds the members of its point in
 * registers and compares all pairs.  ens, bstride, estride, tar, wrow as for mk_ens_sums; gens has batch and member strides
 * gbstride, gestride of its own (elements, a member's [C][H][W] block contiguous) and only the points are written: gaps
 * between the blocks keep what they hold.  Same decomposition and staging as mk_ens_sums; a tile leaves LDS through the
 * mirror image of the staging: per member a scalar head up to that member's own 16-byte boundary, 16-byte stores, a scalar
 * tail.  One launch, no atomics, no workspace, the same bits every run; 64-bit element offsets; B, C <= 65535; fp
 * contraction off.  Every refusal (what mk_ens_sums refuses, for both sides, and E above 16) returns 1 before any launch. */
int mk_ens_crps_bwd(const void* ens, int dtype, long long bstride, long long estride, const float* tar, const float* wrow,
                    const double* gs, void* gens, long long gbstride, long long gestride, int B, int E, int C, int H, int W,
                    void* stream);

/* Forecast products of an ensemble: K planes per sample and selected channel, out [B][K][Cs][H][W] (fp32: out_dtype 0, bf16:
 * 1), from ens [B][E][C][H][W] read as mk_ens_sums reads it (dtype, bstride, estride in elements, a member's [C][H][W] block
 * contiguous, gaps never touched), 2 <= E <= 64, 1 <= K <= 16.  A product's [Cs][H][W] block is contiguous; obstride (sample)
 * and okstride (product) are free, in elements, and what lies between the blocks keeps its bytes.
 * chans: device int32 [Cs], the member channel of output channel j, any order, repeats allowed; NULL: the identity, Cs == C.
 * The grid runs over Cs: a channel that is not selected is never read.  A chans[j] outside [0, C) reads nothing and gives
 * NaN planes.  kinds, orders, fracs: HOST arrays of length K (copied into the kernel's arguments).  Per point, with the
 * members x_e widened to fp64 (exact):
 *   kind 0 mean   m = (sum_e x_e) / E, summed in member order, a division (E equal members x give m = x exactly)
 *   kind 1 std    sqrt(sum_e (x_e - m)^2 / (E - 1)), two-pass about m, fma accumulation, a division; +0 for E equal members
 *   kind 2 order  fma(t, x_(k+1) - x_(k), x_(k)) over the members sorted ascending (ranks from 0), k = orders[i],
 *                 t = fracs[i] in [0, 1); with t == 0 it is x_(k) itself, x_(k+1) is not read and k = E - 1 is legal.
 *                 numpy's `linear` quantile q is k = floor(q (E - 1)), t = q (E - 1) - k
 *   kind 3 above  #{e : x_e > thr[i][j]} / E         kind 4 below  #{e : x_e < thr[i][j]} / E
 *                 compared in fp32 (exact), a tie counts for neither; thr device fp32 [K][Cs], read for these kinds only,
 *                 a NaN threshold gives a NaN plane; one IEEE fp32 division of the two integers
 * Kinds 0 - 2 are formed in fp64 and rounded ONCE to fp32 (a t == 0 order statistic is the member's value, untouched);
 * with scale and shift (device fp32 [Cs], both or neither) the fp32 value v becomes v * scale[j] + shift[j] in fp32, two
 * roundings, contraction off, as the rollout tail applies its emit statistics; kind 1 is multiplied by scale[j] only, kinds 3
 * and 4 are never scaled.  A bf16 output is that fp32 value stored with round to nearest even.  If a member of a point is
 * NaN, all K products of the point are NaN (looked for before the sort, whose min / max drop a NaN); +-inf is out of contract.
 * Decomposition and staging of mk_ens_sums (workgroup = 8 rows of one selected channel of one sample, tiles of 256 points,
 * 128 for E > 32, one point per thread, every member from its own 16-byte boundary); the sorted members go back into the
 * thread's own LDS column, where the table's ranks address them, the K values of a tile into a second [K][TP] LDS region
 * that leaves through the mirror image of the staging, every plane from its own 16-byte boundary.  At most 48 KB of LDS.
 * One launch, no atomics, no workspace, one writer per element, the same bits every run, 64-bit element offsets, B and
 * Cs <= 65535.  Every refusal (sizes, strides below C H W / Cs H W, overlapping samples, alignment, a kind outside 0 ... 4, a
 * rank outside 0 ... E - 1 (E - 2 where t > 0), t outside [0, 1), a count kind without thr, scale without shift) returns 1
 * before any launch. */
int mk_ens_products(const void* ens, int dtype, long long bstride, long long estride, void* out, int out_dtype,
                    long long obstride, long long okstride, const int* chans, const int* kinds, const int* orders,
                    const double* fracs, const float* thr, const float* scale, const float* shift, int B, int E, int C, int Cs,
                    int K, int H, int W, void* stream);

/* ---- latitude interpolation (csrc/grid.hip): P planes [Hs][W] onto Hd destination rows, what GridConverter does between
 * an equiangular archive and a Legendre-Gauss model grid.  Fields are fp32 (dtype 0) or bf16 (1), each side with a dtype, a
 * plane stride and a row stride (elements) of its own; rows are contiguous along W, start at any element-aligned address,
 * and only the W columns of a row are touched.  Tables (device): idx [Hd] int32 local source rows in [0, Hs - 2], wgt [Hd]
 * fp32, any finite value; their contents are not checked here.  With a = x'[p][idx[k]], b = x'[p][idx[k] + 1], d = fl(b - a):
 *   y[p][k] = |wgt[k]| < 0.5 ? fma(wgt[k], d, a) : fma(fl(wgt[k] - 1), d, b)
 * x' = x, or with bias and scale [C] fp32 (both or neither) x' = fl(fl(x - bias[c]) / scale[c]), c = p mod C, an IEEE
 * division.  bf16 widens exactly, the store rounds once.  One launch, no atomics, no workspace, the same bits every run;
 * 64-bit offsets; fp contraction off.  A refusal (null or misaligned pointer, dtype outside the table, Hs < 2, W < 1, a row
 * stride below W, overlapping output planes) returns 1 before any launch. */
int mk_lat_lerp_fwd(const void* x, int xdtype, long long xpstride, long long xrstride, void* y, int ydtype, long long ypstride,
                    long long yrstride, const int* idx, const float* wgt, const float* bias, const float* scale, int C,
                    long long P, int Hs, int Hd, int W, void* stream);
/* The gradient with respect to x, a gather over the transposed table in CSR form: rowptr [Hs + 1], and per term a
 * destination row term_row and a coefficient term_coef (1 - w for the a-term, w for the b-term, each rounded once to fp32
 * from the float64 weight), terms of a source
 * row by ascending destination row, a-term first:
 *   gx[p][j] = (fma chain from 0, in that order, of term_coef[t] * gy[p][term_row[t]]) / scale[p mod C]
 * (scale NULL: no division).  A source row without terms gets zeros.  gy [P][Hd][W], gx [P][Hs][W]; rules as above. */
int mk_lat_lerp_bwd(const void* gy, int gydtype, long long gypstride, long long gyrstride, void* gx, int gxdtype,
                    long long gxpstride, long long gxrstride, const int* rowptr, const int* term_row, const float* term_coef,
                    const float* scale, int C, long long P, int Hs, int Hd, int W, void* stream);
/* Columns of a row one wave of the two kernels takes (the tests choose a width beyond it). */
int mk_lat_lerp_chunk(void);

/* ---- correlated spherical noise (csrc/noise.hip): one step of an isotropic Gaussian random field, drawn straight into the
 * packed spectrum state [L][M][BC] (complex64, BC fastest) that legendre_inv / inverse_packed synthesise.  The reference has
 * no such component (its perturbation is white grid noise); this goes beyond it.  The shard holds degrees l_off ... l_off + L - 1
 * and orders m_off ... m_off + M - 1 of rows row0 ... row0 + BC - 1.  With gl = l_off + l, gm = m_off + m, q = (row0 + bc) >> 1 and
 * T = t + (t_dev ? *t_dev : 0) mod 2^32 (t_dev: a device int32, read by the kernel, so a captured launch draws anew on replay):
 *   words = Philox4x32-10(counter (q, gl, gm, T), key (low, high 32 bits of seed));  the seed is the two's complement long long of
 *           an integer in [0, 2^64).  Row 2q takes words (0, 1) as (a, b), row 2q + 1 words (2, 3)
 *   u1 = ((a >> 8) + 1) 2^-24,  u2 = (b >> 8) 2^-24,  rad = sqrtf(-2 logf(u1)),  (z_re, z_im) = rad (cospi(2 u2), sinpi(2 u2))
 *   xi = gm == 0 ? (s sigma_l[l]) z_re + 0 i : (s fl(sigma_l[l] / sqrt 2)) (z_re + i z_im),   s = row_scale ? row_scale[bc] : 1
 *   phi == 0:     state = xi                       (the old state is not read and may hold NaN)
 *   0 < phi < 1:  state = fl(fl(phi state) + fl(fl(sqrt(1 - phi^2)) xi))        (AR(1) with stationary variance sigma_l^2)
 * and every entry with gl < gm is written as exact zero.  sigma_l [L] and row_scale [BC] (or NULL) are device fp32.  The counter
 * names global indices only: a shard's draw is bitwise the slice of the unsharded draw.  logf, sqrtf and sincospif are the
 * accurate ones (no fast-math), contraction is off.  One thread per (l, m, q), one 16-byte store per pair for even BC, 8-byte
 * stores for odd BC.  One launch, no atomics, no workspace, the same bits every run.  Every refusal (null or not 16-byte
 * aligned state, null sigma_l, L, M or BC below 1, a negative offset, odd or negative row0, q reaching 2^32, phi outside
 * [0, 1), L M ceil(BC / 2) of 2^31 or more: the kernel's thread index is 32-bit) returns 1 before any launch. */
int mk_noise_spectrum(void* state, const float* sigma_l, const float* row_scale, int L, int M, long long BC, int l_off, int m_off,
                      long long row0, long long seed, int t, const int* t_dev, float phi, void* stream);
/* The four Philox words of counter (q, l, m, t) (global indices) under `seed`, computed on the host by the code the kernel
 * runs (csrc/philox.h); l, m and t are taken as their 32 bits (a word above 2^31 travels as a negative int) and out4 receives
 * the words the same way.  q outside [0, 2^32) and a null out4 are refused.  No launch, no GPU needed. */
int mk_noise_words(long long seed, long long q, int l, int m, int t, int* out4);

/* ---- cosine of the solar zenith angle (csrc/zenith.hip), the unpredicted channel of the production configs, from
 * per-time scalars: fp32, all on the device,
 *   eph [n][4] = (sin dec, cos dec, GMST, right ascension; radians),  sin_lat, cos_lat [H],  lon_rad [W],
 *   out [n][H][W] = sin_lat[i] sin dec + (cos_lat[i] cos dec) cos((GMST + lon_rad[j]) - ra)
 * with every product and sum rounded on its own in that order (the file is compiled with fp contraction off: a
 * v_mul and a v_add per point, no fma outside cosf itself) and the accurate cosf, which is the arithmetic of
 * makani/third_party/climt/zenith_angle.py.  A point depends on its (time, row, column) only: a launch on slices of the
 * tables gives the slice of the full field bit for bit.  Any W, any element-aligned out; n == 0 launches nothing.  Writes
 * only; no atomics, allocation, synchronisation or host copy. */
int mk_cos_zenith(const float* eph, const float* sin_lat, const float* cos_lat, const float* lon_rad, float* out, long long n,
                  int H, int W, void* stream);

/* ---- layer norm over the CHANNEL axis of an NCHW field (csrc/chnorm.hip): DistributedLayerNorm
 * (makani/mpu/layer_norm.py:117-155; normalization_layer = "layer_norm", makani/models/networks/sfnonet.py:371-382) without
 * the transposes around nn.LayerNorm.  x [B][C][P] contiguous, P = H W, fp32 (dtype 0) or bf16 (1); per (b, p)
 *   mean = sum_c x / C,  var = sum_c (x - mean)^2 / C (biased, two passes),  rstd = 1 / sqrt(var + eps),
 *   y_c = act(weight[c] (x_c - mean) rstd + bias[c]),  act = exact GELU if fuse_gelu else identity,
 * computed in fp32 and rounded once on the store to y's dtype (0 / 1, independent of x's).  weight, bias fp32 [C], each may
 * be NULL (1 / 0).  stats [B][P][2] = (mean, rstd) fp32 is kept for the backward (NULL: not written).  Any B, C, P >= 1 and any
 * element-aligned pointers: 16-byte vectors when P is a multiple of 16 / sizeof(x element) and x, y (gy, gx) are 16-byte
 * aligned, single elements otherwise; a pixel tile over all channels stays in LDS between its uses while it fits, else it is
 * read again (L2).  x is read once and y written once from / to HBM.  The channel sums of a pixel are formed in an order
 * that depends on C only, so a launch on a spatial slice gives the bits of the slice of the full result.
 * Backward: gy [B][C][P] fp32 / bf16 (its own dtype), with xh = (x - mean) rstd, g = gy (fused: gy gelu'(weight xh + bias),
 * recomputed), s1 = sum_c weight g, s2 = sum_c weight g xh:
 *   gx_c = rstd (weight[c] g_c - s1 / C - xh_c s2 / C)   in x's dtype,
 *   gwb [2][C] fp32:  row 0 = sum_{b,p} g_c xh_c (weight gradient),  row 1 = sum_{b,p} g_c (bias gradient);
 * gwb NULL: not formed.  Deterministic (no atomics): per-workgroup fp32 partials in `workspace`
 * (mk_chan_layernorm_workspace(B, C, P) floats, no need to clear it), added in a fixed order in fp64 by a finishing launch.
 * No allocation, synchronisation or host copy; the launch configuration depends on the shape and dtypes only. */
long long mk_chan_layernorm_workspace(int B, int C, long long P);
int mk_chan_layernorm_fwd(const void* x, int x_dtype, const float* weight, const float* bias, void* y, int y_dtype,
                          float* stats, int B, int C, long long P, float eps, int fuse_gelu, void* stream);
int mk_chan_layernorm_bwd(const void* x, int x_dtype, const void* gy, int gy_dtype, const float* stats, const float* weight,
                          const float* bias, void* gx, float* workspace, float* gwb, int B, int C, long long P, int fuse_gelu,
                          void* stream);

/* ---- per-degree power of a packed spectrum (csrc/specnorm.hip): the degree sums of GeometricH1Loss
 * (makani/utils/losses.py:306-318) without the public layout.  c [L][M][BC] complex64 (the private spectrum; rows with
 * l_off + l < m_off + m may hold anything, they are never loaded), l_off / m_off the shard's global offsets as for
 * mk_spec_unpack:
 *   P[l][bc] = sum_m w(m_off + m) |c[l][m][bc]|^2,   w(0) = 1, w(m > 0) = 2,   P [L][BC] fp64.
 * re and im are converted to double before squaring and added in double in ascending m, in chunks of a fixed number of
 * local orders that a finishing launch adds in order: deterministic (no atomics), independent of l_off, so the rows of an
 * l slice carry the bits of the same rows of the whole; the sums add up over m shards.  Any L, M, BC >= 1.  No allocation,
 * synchronisation or host copy: `workspace` holds mk_degree_power_workspace(L, M, BC) doubles (no need to clear it).
 * Backward, gP [L][BC] fp64 on the device (the upstream gradient of P):
 *   gc[l][m][bc] = 2 w(m_off + m) gP[l][bc] c[l][m][bc]   (product in double, rounded once to fp32),
 * exact zeros where l_off + l < m_off + m: the complex gradient in torch's convention (d/d re + i d/d im), in c's layout. */
long long mk_degree_power_workspace(int L, int M, int BC);
int mk_degree_power(const float* c, double* workspace, double* P, int L, int M, int BC, int l_off, int m_off, void* stream);
int mk_degree_power_bwd(const float* c, const double* gP, float* gc, int L, int M, int BC, int l_off, int m_off, void* stream);

/* ---- the spectral ensemble CRPS (csrc/spec_crps.hip): the CRPS terms of the spherical-harmonic coefficients of E ensemble
 * members against a target, summed per degree, and their gradient with respect to the members.  Not in the reference.
 *   cp [L][M][B E C] complex64, row (b E + e) C + c: forward_packed of a prediction [B E, C, H, W], member fastest;
 *   ct [L][M][B C]   complex64, row b C + c;   l_off / m_off the shard's global offsets as for mk_degree_power.
 * Rows with l_off + l < m_off + m may hold anything, they are never loaded.  For every stored coefficient, every (b, c) and
 * each component k in {re, im} taken as a real number, with x_e the members and y the target widened to fp64 (exact),
 *   a_k = (1/E) sum_e |x_e - y|,      g_k = (1/E^2) sum_{e,f} |x_e - x_f|,
 *   S[l][b C + c][0] = sum_m w(m_off + m) (a_re + a_im),   S[l][b C + c][1] = sum_m w(m_off + m) (g_re + g_im),
 *   w(0) = 1, w(m > 0) = 2,   S [L][B C][2] fp64.
 * The order of the fp64 additions: per coefficient and component sum_e |x_e - y| in ascending e and sum_{e < f} |x_e - x_f| in
 * lexicographic (e, f); re + im; acc += w (.) in ascending m within chunks of a fixed number of local orders; the chunks
 * of (l, b, c) in ascending order by a finishing launch, which multiplies by 1 / E and 2 / E^2.  Deterministic (no atomics),
 * independent of l_off: the rows of an l slice carry the bits of the same rows of the whole; the sums add up over m shards.
 * A NaN component in a member or in the target makes both sums of that (b, c, l) NaN.  E is 2 ... 16.  Two launches, no
 * allocation, synchronisation or host copy: `workspace` holds mk_spec_crps_workspace(L, M, B C) doubles (no need to clear it).
 * Backward, gS [L][B C][2] fp64 on the device (the upstream gradient of S): with L_e = #{f : x_f < x_e} and
 * G_e = #{f : x_f > x_e} per component,
 *   gcp[l][m][(b E + e) C + c] (component k) = w(m_off + m) (gS0 sgn(x_e - y) / E + gS1 2 (L_e - G_e) / E^2),   sgn(0) = 0,
 * the gradient of the all-pairs expression (abs'(0) = 0) in torch's complex convention (d/d re + i d/d im): tied members get
 * equal values, the zero imaginary parts of m = 0 an exact zero.  Comparisons in fp32 (exact), counts integers, the value
 * formed in fp64 and rounded once to fp32.  Exact zeros where l_off + l < m_off + m.  A NaN component in a member or in the
 * target makes both components of every member's gradient of that coefficient NaN.  No gradient goes to the target.  One
 * launch, no workspace, no atomics.  Both: 64-bit offsets, fp contraction off; every refusal (null pointer, a buffer not
 * 8-byte aligned, E outside 2 ... 16, sizes below 1, negative offsets, L M B E C of 2^38 or more) returns 1 before any launch. */
long long mk_spec_crps_workspace(int L, int M, int BC);
int mk_spec_crps_sums(const float* cp, const float* ct, double* workspace, double* S, int L, int M, int B, int E, int C, int l_off,
                      int m_off, void* stream);
int mk_spec_crps_bwd(const float* cp, const float* ct, const double* gS, float* gcp, int L, int M, int B, int E, int C, int l_off,
                     int m_off, void* stream);

/* ---- scaled-dot-product attention (csrc/attn.hip): F.scaled_dot_product_attention of the ViT attention module
 * (makani/models/networks/vit.py:44-55), non-causal, no mask, no dropout.  bf16 operands, fp32 scores, softmax and accumulators:
 *   o[b,h,i,:] = sum_j P[i,j] v[b,h,j,:],   P = softmax_j(scale q[b,h,i,:] . k[b,h,j,:]),   lse[b,h,i] = ln sum_j exp(scale s_ij).
 * Every bf16 tensor is a base pointer (16-byte aligned) and three element strides (batch, head, token), each a non-negative
 * multiple of 8, the token stride at least D; the D axis is contiguous.  `strides` holds them in the order of the pointer
 * arguments, three per tensor, and is read on the host during the call.  q, k, v may so be the three views of one
 * [B][N][3][H][D] projection output, o a [B][N][H D] buffer, and dq, dk, dv the views of one [B][N][3][H][D] gradient.
 * D a multiple of 16 in 16 ... 128 (zero-padded on chip to 64 or 128; a padded element is never read or written); any
 * Nq, Nk >= 1, independent.  lse, delta [B][H][Nq] fp32 contiguous; mk_attn_fwd takes lse == NULL (nothing stored).
 * P (fwd, dkv) and dS = P o (dO V^T - delta) (dkv, dq) are rounded to bf16 (nearest even) before their second products;
 * delta = rowsum(dO o O) is formed from the stored bf16 o.  dq = scale dS K, dk = scale dS^T Q, dv = P^T dO.
 * One workgroup per (batch, head, tile of 128 queries) in fwd and dq, per (batch, head, tile of 128 keys) in dkv; nothing is
 * summed across workgroups: no atomics, no waiting on another workgroup, the same inputs give the same bits.  Each call is
 * one launch on `stream`, allocates nothing, does not synchronise and can be captured.  Unsupported D, strides or alignment
 * return code 1 before any launch.
 * mk_attn_info: tiles[6] = (query tile, key tile) of fwd, of dkv and of dq for head size D. */
int mk_attn_info(int D, int* tiles);
int mk_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int Nq, int Nk, int D,
                const long long* strides, float scale, void* stream);
int mk_attn_bwd_delta(const void* o, const void* dO, float* delta, int B, int H, int Nq, int D, const long long* strides,
                      void* stream);
int mk_attn_bwd_dkv(const void* q, const void* k, const void* v, const void* dO, const float* lse, const float* delta, void* dk,
                    void* dv, int B, int H, int Nq, int Nk, int D, const long long* strides, float scale, void* stream);
int mk_attn_bwd_dq(const void* q, const void* k, const void* v, const void* dO, const float* lse, const float* delta, void* dq,
                   int B, int H, int Nq, int Nk, int D, const long long* strides, float scale, void* stream);

/* ---- the same attention with fp32 operands on the bf16x3 arithmetic (csrc/x3_attn.hip): F.scaled_dot_product_attention of the
 * ViT attention module (makani/models/networks/vit.py:44-55) when the model runs in plain fp32 (amp_mode none).  fp32 q, k, v,
 * dO in, fp32 o, lse, delta, dq, dk, dv out; the formulas and the argument shape of mk_attn_*: a base pointer (16-byte aligned)
 * and three element strides (batch, head, token) per tensor, each a non-negative multiple of 4, the token stride at least D, the D
 * axis contiguous; `strides` in the order of the pointer arguments, read on the host during the call.  q, k, v may be the three
 * views of one fp32 [B][N][3][H][D] projection output, o a [B][N][H D] buffer, dq, dk, dv the views of one [B][N][3][H][D] gradient.
 * D a multiple of 16 in 16 ... 64 (zero-padded on chip to 64; a padded element is never read or written); any Nq, Nk >= 1,
 * independent.  lse, delta [B][H][Nq] fp32 contiguous; mk_attn_x3_fwd takes lse == NULL (nothing stored).
 * Every operand of the two forward and the five backward matrix products is split exactly into three bf16 pieces by truncation
 * (x = h + m + l) and a product is the six piece products of weight >= 2^-16 on v_mfma_f32_32x32x16_bf16, accumulated in fp32;
 * P and dS = P o (dO V^T - delta) are fp32 and are split in registers before their second products; scores, online softmax, row
 * sums, lse and delta = rowsum(dO o O) (from the stored fp32 o) are fp32.
 * One workgroup per (batch, head, tile of 128 queries) in fwd and dq, per (batch, head, tile of 128 keys) in dkv; nothing is
 * summed across workgroups: no atomics, no waiting on another workgroup, the same inputs give the same bits.  Each call is
 * one launch on `stream`, allocates nothing, does not synchronise and can be captured.  Unsupported D, strides, alignment or
 * sizes past the 32-bit row range return code 1 before any launch.
 * mk_attn_x3_info (no device needed): tiles[6] = (query tile, key tile) of fwd, of dkv and of dq for head size D. */
int mk_attn_x3_info(int D, int* tiles);
int mk_attn_x3_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int H, int Nq, int Nk, int D,
                   const long long* strides, float scale, void* stream);
int mk_attn_x3_bwd_delta(const float* o, const float* dO, float* delta, int B, int H, int Nq, int D, const long long* strides,
                         void* stream);
int mk_attn_x3_bwd_dkv(const float* q, const float* k, const float* v, const float* dO, const float* lse, const float* delta,
                       float* dk, float* dv, int B, int H, int Nq, int Nk, int D, const long long* strides, float scale, void* stream);
int mk_attn_x3_bwd_dq(const float* q, const float* k, const float* v, const float* dO, const float* lse, const float* delta,
                      float* dq, int B, int H, int Nq, int Nk, int D, const long long* strides, float scale, void* stream);

/* ---- layer norm over the TRAILING axis with the residual add fused in (csrc/toknorm.hip): nn.LayerNorm of the ViT blocks
 * (makani/models/networks/vit.py:86-118) and nn.LayerNorm((h, w)) of AFNO (afnonet.py:249-250).  `rows` rows of L >= 1
 * contiguous elements; every tensor has its own dtype (0 = fp32, 1 = bf16) and element row stride ld >= L.  Per row
 *   s = x + r (added in fp32; r NULL: s = x),  mean = sum s / L,  var = sum (s - mean)^2 / L (biased, two passes over the
 *   on-chip row),  rstd = 1 / sqrt(var + eps),  v = weight (s - mean) rstd + bias   in fp32,
 * weight, bias fp32 [L], each may be NULL (1 / 0).  Outputs, each may be NULL but not both y and y2: y = v rounded once to
 * y_dtype; y2 = the same fp32 v rounded once to bf16 (the operand of the next linear under autocast); s_out = s in s_dtype;
 * stats [rows][2] = (mean, rstd) fp32.
 * Backward: s is recomputed from x and r (the forward need not have stored it); gy (its dtype), gy2 (bf16) and gs (the
 * gradient of s_out, its dtype) may each be NULL.  With g = gy + gy2 in fp32, xh = (s - mean) rstd, s1 = sum weight g,
 * s2 = sum weight g xh over the row:
 *   gx = rstd (weight g - s1 / L - xh s2 / L) + gs   in x's dtype and ld;  gr (NULL: not written) the same values in r's;
 *   gwb [2][L] fp32 (NULL: not formed):  row 0 = sum_rows g xh,  row 1 = sum_rows g.
 * gwb uses no atomics: per-workgroup fp32 partials in `workspace` (mk_token_layernorm_workspace(rows, L) floats, no need to
 * clear it), added in a fixed order in fp64 by a finishing launch.
 * Any rows, L >= 1 and any element-aligned pointers and strides: 16-byte vectors when L is a multiple of 8 and every pointer
 * and row stride is a multiple of 16 bytes, single elements otherwise.  Rows of up to 2048 elements are held in the
 * registers of one wavefront; longer ones by a workgroup in LDS while they fit (40 944 elements forward, 20 472
 * backward), and are read again (L2) beyond that.  x and r are read once and every output is written once from / to HBM.
 * The sums of a row are formed in an order that depends on L only -- not on the alignment or on the row's place -- so a
 * launch on a subset of the rows gives the bits of that subset (y, gx, stats), and the same inputs give the same bits.
 * Columns L ... ld - 1 of an output are never written.  No allocation, synchronisation or host copy; can be captured; the
 * launch configuration depends on the shape, the dtypes and the alignment only. */
long long mk_token_layernorm_workspace(long long rows, long long L);
int mk_token_layernorm_fwd(const void* x, int x_dtype, long long x_ld, const void* r, int r_dtype, long long r_ld,
                           const float* weight, const float* bias, void* y, int y_dtype, long long y_ld, void* y2, long long y2_ld,
                           void* s_out, int s_dtype, long long s_ld, float* stats, long long rows, long long L, float eps,
                           void* stream);
int mk_token_layernorm_bwd(const void* x, int x_dtype, long long x_ld, const void* r, int r_dtype, long long r_ld, const void* gy,
                           int gy_dtype, long long gy_ld, const void* gy2, long long gy2_ld, const void* gs, int gs_dtype,
                           long long gs_ld, const float* stats, const float* weight, void* gx, void* gr, float* workspace,
                           float* gwb, long long rows, long long L, void* stream);

/* ---- token-major linear layers (csrc/toklinear.hip): nn.Linear on [R rows][I features] activations with [O][I] weights, the
 * qkv / proj / fc1 / fc2 / head products of the ViT and of the "traditional" MLP / EncoderDecoder.  bf16 operands, products on
 * bf16 MFMA, fp32 accumulation.  Every matrix is a 16-byte-aligned base pointer and a row stride in elements (a multiple of
 * 8, at least the row length); the feature axis is contiguous.  I and O are multiples of 8, R >= 1 is any count and row
 * offsets are 64-bit.  A ragged last tile loads zeros and stores nothing in R, O and I: columns past a row's length are
 * neither read nor written.  Each entry point validates and returns code 1 before any launch; it is one launch on `stream`
 * (mk_token_linear_wgrad: two when it uses more than one slab), allocates nothing, does not synchronise and can be captured.
 * Nothing is summed across workgroups by atomics and no workgroup waits on another: the same inputs give the same bits.
 * mk_token_linear_info: tiles[6] = row tile, output tile, contraction step of the GEMM; O tile, I tile, token step of the
 *   weight gradient.  Needs no device.
 * mk_token_linear_pack: w ([O][I], w_dtype 0 = fp32, 1 = bf16) rounded to nearest even into the bf16 image out [O][I], or with
 *   `transpose` out [I][O].
 * mk_token_linear_fwd: acc[r][o] = sum_i x[r][i] w[o][i], x bf16 [R][I], w a bf16 image [O][I]; bias fp32 [O] (16-byte
 *   aligned) or NULL.  The epilogue is selected by the non-NULL pointers, anything else is code 1:
 *     y                      y = bf16(acc + bias)
 *     act (and pre)          pre = bf16(acc + bias), stored when given; act = bf16(gelu(float(pre))), exact erf GELU: act has the
 *                            same bits with and without pre
 *     addend and out_f32     out_f32 = addend + float(bf16(acc + bias)), both fp32 [R][O]; no bf16 output
 *     y and aux (no bias)    y = bf16(acc * gelu'(float(aux))), aux bf16 [R][O]: with x = the gradient of fc2's output and w the
 *                            transposed image of fc2's weight this is the gradient of fc1's pre-activation, rounded once
 * mk_token_linear_gelu_grad: out = bf16(float(g) * gelu'(float(pre))), all bf16 [R][O].
 * mk_token_linear_wgrad: dw[o][i] = sum_r dy[r][o] x[r][i] (fp32 [O][I]) and, db not NULL, db[o] = sum_r dy[r][o] (fp32 [O],
 *   16-byte aligned); dy bf16 [R][O], x bf16 [R][I].  The token steps are split into `slabs` (1 ... 64) groups of whole steps;
 *   each (slab, O tile, I tile) workgroup stores an fp32 partial panel into `workspace` and a second launch adds the panels,
 *   and the slabs' column sums for db, in slab order in fp32.  One slab stores the results directly (one launch, no
 *   workspace).  slabs = 0 chooses: one workgroup per compute unit where the tiles alone give fewer, no slab shorter than 4
 *   token steps and none empty.  mk_token_linear_wgrad_workspace: the bytes `workspace` must hold (no need to clear it; 16-byte
 *   aligned), -1 for sizes the kernels refuse. */
int mk_token_linear_info(int* tiles);
int mk_token_linear_pack(const void* w, int w_dtype, long long ldw, void* out, long long ldo, int O, int I, int transpose,
                         void* stream);
int mk_token_linear_fwd(const void* x, long long ldx, const void* w, long long ldw, const float* bias, void* y, long long ldy,
                        void* act, long long ldact, void* pre, long long ldpre, const float* addend, long long ldadd,
                        float* out_f32, long long ldout, const void* aux, long long ldaux, long long R, int O, int I,
                        void* stream);
int mk_token_linear_gelu_grad(const void* g, long long ldg, const void* pre, long long ldpre, void* out, long long ldout,
                              long long R, int O, void* stream);
long long mk_token_linear_wgrad_workspace(long long R, int O, int I, int slabs);
int mk_token_linear_wgrad(const void* dy, long long lddy, const void* x, long long ldx, float* dw, long long lddw, float* db,
                          void* workspace, long long R, int O, int I, int slabs, void* stream);

/* ---- token-major linear layers on fp32 rows (csrc/x3_toklinear.hip): the same nn.Linear products outside autocast -- the
 * reference's fp32 run (`amp_mode none`): qkv / proj / fc1 / fc2 / head of the ViT (models/networks/vit.py:14-104), the Mlp of
 * AFNOv1 (models/networks/afnonet.py:26-44) and the "traditional" MLP / EncoderDecoder (layers.py:86-216) -- fp32-accurate on the bf16x3
 * engine (csrc/x3_engine.h) instead of a vendor fp32 GEMM.  Every matrix is fp32, a 16-byte-aligned base pointer and a row
 * stride in elements (a multiple of 4, at least the row length); the feature axis is contiguous.  I and O are multiples of 4,
 * R >= 1.  The 32-bit offsets of a tile need 129 ld 4 < 2^31 for operands read row-major over the contraction (x, and w with
 * w_kmajor 0) and 33 ld 4 < 2^31 for k-major ones (w with w_kmajor 1, dy and x of the weight gradient).  A ragged last tile
 * loads zeros and stores nothing; columns past a row's length are neither read nor written.  Each entry point validates
 * and returns nonzero with a message before any launch; all launches go on `stream`, nothing is allocated or synchronised, so
 * it can be captured.  No atomics: the same inputs give the same bits.
 * mk_token_linear_x3_info: t[3] = tile rows, tile columns, k-step.  Needs no device.
 * mk_token_linear_x3_fwd (F.linear, and F.linear's data gradient): I is the contraction length, O the output's row length,
 *     w_kmajor 0:  acc[r][o] = sum_k x[r][k] w[o w_ld + k]      w [O][I]
 *     w_kmajor 1:  acc[r][o] = sum_k x[r][k] w[k w_ld + o]      w [I][O]: with x = the output's gradient the data gradient,
 *                                                               from the weight as it is stored
 *   then, in this order, whatever is given:  v = acc + bias[o];  pre = v;  v = gelu(v) if act (exact erf form);  v += addend[r][o];
 *   v *= gelu'(aux[r][o]);  y = v.  bias fp32 [O] (16-byte aligned); y, pre, addend, aux [R][O].  Accepted combinations
 *   (bias optional unless stated): y alone;  act = 1 with or without pre (fc1);  addend with act = 0 (fc2 with the block's
 *   residual, the patch embedding with pos_embed);  aux with act = 0 and without bias, pre or addend (with w_kmajor 1: fc2's
 *   data gradient times gelu'(pre) = the gradient of fc1's pre-activation).  pre needs act = 1.  Anything else is refused.
 * mk_token_linear_x3_wgrad (the weight / bias gradient of F.linear): dw[o][i] = sum_r dy[r][o] x[r][i], dy [R][O], x [R][I],
 *   dw [O][I].  The tokens are cut into `slabs` (1 ... 64; fewer where R has fewer 32-row steps) ranges of whole steps, each
 *   into an fp32 panel in `ws`; a second launch adds the panels in slab order.  One slab stores dw directly.  slabs = 0 chooses:
 *   about three workgroups per compute unit, no slab shorter than 4 steps.  db (fp32 [O], 16-byte aligned, or NULL):
 *   db[o] = sum_r dy[r][o], float64 partials of 128 rows (one more launch) added in row order by the finishing launch.
 *   mk_token_linear_x3_wgrad_workspace: the bytes `ws` must hold (16-byte aligned, no need to clear it; NULL is accepted when
 *   there is one slab and no db), -1 for sizes the kernels refuse. */
int mk_token_linear_x3_info(int* t);
int mk_token_linear_x3_fwd(const float* x, long long x_ld, const float* w, long long w_ld, int w_kmajor, const float* bias,
                           float* y, long long y_ld, float* pre, long long pre_ld, const float* addend, long long addend_ld,
                           const float* aux, long long aux_ld, int act, long long R, int O, int I, void* stream);
long long mk_token_linear_x3_wgrad_workspace(long long R, int O, int I, int slabs);
int mk_token_linear_x3_wgrad(const float* dy, long long dy_ld, const float* x, long long x_ld, float* dw, long long dw_ld,
                             float* db, void* ws, long long R, int O, int I, int slabs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAKANI_AMD_H */
