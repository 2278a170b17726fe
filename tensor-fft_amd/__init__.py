"""tensor-fft_amd: MI355X (gfx950) tensor-core FFT, host side.

Import name: ``tensor_fft_amd`` (see ``tensor_fft_amd.py`` at the repository
root; the directory carries the upstream project's hyphen).

Thirteen layers, all thin:

* :mod:`.capi` — ctypes binding of the C ABI ``include/tfft.h`` in
  ``libtfft.so`` (hand-written HIP, built in-tree by ``__graft_entry__.build``).
  There is NO CPU or PyTorch fallback: if the library is missing or the device is
  not gfx950, calls raise.
* :mod:`.conv` — ctypes binding of the FFT convolution add-on ``include/tfft_conv.h`` in
  ``libtfft_conv.so`` (layered on ``libtfft.so``; same rule: no fallback).
* :mod:`.lconv` — ctypes binding of the causal real convolution add-on ``include/tfft_lconv.h`` in
  ``libtfft_lconv.so`` (layered on the other two; same rule: no fallback).
* :mod:`.gconv` — ctypes binding of the gated causal convolution add-on ``include/tfft_gconv.h`` in
  ``libtfft_gconv.so`` (layered on ``libtfft_conv.so`` and ``libtfft.so``; same rule: no fallback).
* :mod:`.sconv` — ctypes binding of the overlap-save causal convolution add-on ``include/tfft_sconv.h`` in
  ``libtfft_sconv.so`` (any sequence length in one kernel; layered on ``libtfft_conv.so`` and ``libtfft.so``; no fallback).
* :mod:`.bconv` — ctypes binding of the gradient add-on ``include/tfft_bconv.h`` in ``libtfft_bconv.so`` (the input and the tap
  gradient of the overlap-save convolution, and the ``torch.autograd`` hook over them; layered on ``libtfft_conv.so`` and
  ``libtfft.so``; no fallback).
* :mod:`.gsconv` — ctypes binding of the gated overlap-save convolution add-on ``include/tfft_gsconv.h`` in ``libtfft_gsconv.so``
  (the gated operator of :mod:`.gconv` at any sequence length in one kernel; layered on ``libtfft_conv.so`` and ``libtfft.so``; no
  fallback).
* :mod:`.gbconv` — ctypes binding of the gated gradient add-on ``include/tfft_gbconv.h`` in ``libtfft_gbconv.so`` (the gradients of
  the gated overlap-save convolution, and the ``torch.autograd`` hook over them and :mod:`.gsconv`; layered on ``libtfft_conv.so``
  and ``libtfft.so``; no fallback).
* :mod:`.cconv` — ctypes binding of the carried convolution add-on ``include/tfft_cconv.h`` in ``libtfft_cconv.so`` (the plans of
  :mod:`.sconv` and :mod:`.bconv` on a chunk of a longer sequence, with the history in front of x and the future behind g read in
  place, and the ``torch.autograd`` hook over them; layered on ``libtfft_conv.so`` and ``libtfft.so``; no fallback).
* :mod:`.stft` — ctypes binding of the short-time Fourier transform add-on ``include/tfft_stft.h`` in ``libtfft_stft.so`` (hopped,
  windowed frames of 4096 samples of long real signals to half spectra in one kernel; layered on ``libtfft_conv.so`` and
  ``libtfft.so``; no fallback).
* :mod:`.istft` — ctypes binding of the inverse short-time Fourier transform add-on ``include/tfft_istft.h`` in ``libtfft_istft.so``
  (half spectra of hopped frames back to real signals: a one-pass C2R of every frame and a windowed overlap-add in a fixed order;
  layered on ``libtfft_conv.so`` and ``libtfft.so``; no fallback).
* :mod:`.stftn` — ctypes binding of the short-frame STFT add-on ``include/tfft_stftn.h`` in ``libtfft_stftn.so`` (the plans of
  :mod:`.stft` at the frame lengths 512, 1024 and 2048, one kernel each; layered on ``libtfft_conv.so`` and ``libtfft.so``; no
  fallback).
* :mod:`.istftn` — ctypes binding of the short-frame inverse STFT add-on ``include/tfft_istftn.h`` in ``libtfft_istftn.so`` (the
  plans of :mod:`.istft` at the frame lengths 512, 1024 and 2048; layered on ``libtfft_conv.so`` and ``libtfft.so``; no fallback).
* :mod:`.spec` — ctypes binding of the spectrogram add-on ``include/tfft_spec.h`` in ``libtfft_spec.so`` (power spectrograms and band
  energies, mel among them, of the frames of :mod:`.stftn` in one kernel; layered on ``libtfft_conv.so`` and ``libtfft.so``; no
  fallback), the host-side ``Bands`` container and the mel filterbank.
* :mod:`.mistftn` — ctypes binding of the masked short-frame inverse STFT add-on ``include/tfft_mistftn.h`` in ``libtfft_mistftn.so``
  (the plans of :mod:`.istftn` with a real mask inside the merge, per frame or per bin; layered on ``libtfft_conv.so`` and
  ``libtfft.so``; no fallback), and :mod:`.stft_autograd`, the ``torch.autograd`` hooks of ``short_stft`` and ``power_spectrogram``
  whose backward passes are raw-sum masked plans.
* :mod:`.reference_api` — the reference's own host interface for this path
  (``CreatePlan``, ``PlanWorksOnDevice``, ``GetMaxNoOptInSharedMem``,
  ``DataHandler``, ``DataBatchHandler``, ``ComputeFFT``; reference
  src/base/Plan.h, DataHandler.h, ComputeFFT.h) with the same names, argument
  meaning and error behaviour, on top of :mod:`.capi`. PyTorch supplies device
  memory and streams only.
"""
from .capi import (TfftError, TfftPlan, TfftPlan2D, TfftRealPlan, device_check, irfft, rfft, rplan_cache_clear, rplan_describe, rplan_spectrum_pitch, kernel_list, lib_path, load_library, plan_cache_policy,  # noqa: F401
                   plan_default_variant, plan_describe, ref_create_plan, synth_uniform, transposed_n2, tuning_add, tuning_clear,
                   tuning_load, tuning_query, variant_check)
from .conv import (TfftConvPlan, conv_cache_clear, conv_describe, conv_filter_slot, conv_lib_path, fftconv,  # noqa: F401
                   load_conv_library)
from .lconv import (TfftCausalConvPlan, causal_conv, lconv_cache_clear, lconv_describe, lconv_fft_length, lconv_lib_path,  # noqa: F401
                    lconv_spectrum_host, load_lconv_library)
from .gconv import (TfftGatedConvPlan, gated_causal_conv, gconv_cache_clear, gconv_describe, gconv_fft_length, gconv_lib_path,  # noqa: F401
                    gconv_spectrum_host, load_gconv_library)
from .sconv import (TfftLongConvPlan, load_sconv_library, long_causal_conv, sconv_cache_clear, sconv_describe, sconv_geometry,  # noqa: F401
                    sconv_lib_path)
from .bconv import (TfftLongConvGradPlan, bconv_cache_clear, bconv_describe, bconv_geometry, bconv_lib_path,  # noqa: F401
                    differentiable_long_causal_conv, load_bconv_library, long_causal_conv_input_grad, long_causal_conv_tap_grad)
from .gsconv import (TfftGatedLongConvPlan, gated_long_causal_conv, gsconv_cache_clear, gsconv_describe, gsconv_geometry,  # noqa: F401
                     gsconv_lib_path, load_gsconv_library)
from .gbconv import (TfftGatedLongConvGradPlan, differentiable_gated_long_causal_conv, gated_long_causal_conv_input_grad,  # noqa: F401
                     gated_long_causal_conv_tap_grad, gbconv_cache_clear, gbconv_describe, gbconv_geometry, gbconv_lib_path,
                     load_gbconv_library)
from .cconv import (TfftChunkedConvGradPlan, TfftChunkedConvPlan, cconv_cache_clear, cconv_describe, cconv_geometry, cconv_lib_path,  # noqa: F401
                    chunked_causal_conv, chunked_causal_conv_input_grad, chunked_causal_conv_tap_grad,
                    differentiable_chunked_causal_conv, load_cconv_library, next_history)
from .gcconv import (TfftGatedChunkedConvGradPlan, TfftGatedChunkedConvPlan, differentiable_gated_chunked_causal_conv,  # noqa: F401
                     gated_chunked_causal_conv, gated_chunked_causal_conv_input_grad, gated_chunked_causal_conv_tap_grad,
                     gcconv_cache_clear, gcconv_describe, gcconv_geometry, gcconv_lib_path, load_gcconv_library)
from .stft import (StftOpts, TfftStftPlan, load_stft_library, stft, stft_cache_clear, stft_describe, stft_geometry,  # noqa: F401
                   stft_lib_path)
from .istft import (IstftOpts, TfftIstftPlan, istft, istft_cache_clear, istft_describe, istft_geometry, istft_lib_path,  # noqa: F401
                    load_istft_library)
from .stftn import (StftNOpts, TfftShortStftPlan, load_stftn_library, short_stft, stftn_cache_clear, stftn_describe,  # noqa: F401
                    stftn_geometry, stftn_lib_path)
from .istftn import (IstftNOpts, TfftShortIstftPlan, istftn_cache_clear, istftn_describe, istftn_geometry, istftn_lib_path,  # noqa: F401
                     load_istftn_library, short_istft)
from .spec import (Bands, SpecOpts, TfftSpectrogramPlan, band_spectrogram, bands_from_dense, load_spec_library, mel_bands,  # noqa: F401
                   mel_filterbank, power_spectrogram, spec_cache_clear, spec_describe, spec_geometry, spec_lib_path)
from .mistftn import (MaskedIstftNOpts, TfftMaskedIstftPlan, load_mistftn_library, mask_buffer, masked_istft, mistftn_cache_clear,  # noqa: F401
                      mistftn_describe, mistftn_geometry, mistftn_lib_path)
from .stft_autograd import differentiable_power_spectrogram, differentiable_short_stft, stft_autograd_cache_clear  # noqa: F401
from .reference_api import (  # noqa: F401
    ComputeFFT,
    CreatePlan,
    DataBatchHandler,
    DataHandler,
    GetMaxNoOptInSharedMem,
    Mode_256,
    Mode_4096,
    Plan,
    PlanWorksOnDevice,
)

__all__ = [
    "TfftError", "TfftPlan", "TfftPlan2D", "TfftRealPlan", "device_check", "irfft", "rfft", "rplan_cache_clear", "rplan_describe", "rplan_spectrum_pitch", "lib_path", "load_library", "plan_cache_policy", "plan_default_variant", "plan_describe", "ref_create_plan",
    "synth_uniform", "transposed_n2", "variant_check", "kernel_list", "tuning_add", "tuning_clear", "tuning_load", "tuning_query",
    "TfftConvPlan", "conv_cache_clear", "conv_describe", "conv_filter_slot", "conv_lib_path", "fftconv", "load_conv_library",
    "TfftCausalConvPlan", "causal_conv", "lconv_cache_clear", "lconv_describe", "lconv_fft_length", "lconv_lib_path", "lconv_spectrum_host",
    "load_lconv_library",
    "TfftGatedConvPlan", "gated_causal_conv", "gconv_cache_clear", "gconv_describe", "gconv_fft_length", "gconv_lib_path", "gconv_spectrum_host",
    "load_gconv_library",
    "TfftLongConvPlan", "load_sconv_library", "long_causal_conv", "sconv_cache_clear", "sconv_describe", "sconv_geometry", "sconv_lib_path",
    "TfftLongConvGradPlan", "bconv_cache_clear", "bconv_describe", "bconv_geometry", "bconv_lib_path", "differentiable_long_causal_conv",
    "load_bconv_library", "long_causal_conv_input_grad", "long_causal_conv_tap_grad",
    "TfftGatedLongConvPlan", "gated_long_causal_conv", "gsconv_cache_clear", "gsconv_describe", "gsconv_geometry", "gsconv_lib_path",
    "load_gsconv_library",
    "TfftGatedLongConvGradPlan", "differentiable_gated_long_causal_conv", "gated_long_causal_conv_input_grad",
    "gated_long_causal_conv_tap_grad", "gbconv_cache_clear", "gbconv_describe", "gbconv_geometry", "gbconv_lib_path", "load_gbconv_library",
    "TfftChunkedConvGradPlan", "TfftChunkedConvPlan", "cconv_cache_clear", "cconv_describe", "cconv_geometry", "cconv_lib_path",
    "chunked_causal_conv", "chunked_causal_conv_input_grad", "chunked_causal_conv_tap_grad", "differentiable_chunked_causal_conv",
    "load_cconv_library", "next_history",
    "TfftGatedChunkedConvGradPlan", "TfftGatedChunkedConvPlan", "differentiable_gated_chunked_causal_conv", "gated_chunked_causal_conv",
    "gated_chunked_causal_conv_input_grad", "gated_chunked_causal_conv_tap_grad", "gcconv_cache_clear", "gcconv_describe", "gcconv_geometry",
    "gcconv_lib_path", "load_gcconv_library",
    "StftOpts", "TfftStftPlan", "load_stft_library", "stft", "stft_cache_clear", "stft_describe", "stft_geometry", "stft_lib_path",
    "IstftOpts", "TfftIstftPlan", "istft", "istft_cache_clear", "istft_describe", "istft_geometry", "istft_lib_path", "load_istft_library",
    "StftNOpts", "TfftShortStftPlan", "load_stftn_library", "short_stft", "stftn_cache_clear", "stftn_describe", "stftn_geometry",
    "stftn_lib_path",
    "IstftNOpts", "TfftShortIstftPlan", "istftn_cache_clear", "istftn_describe", "istftn_geometry", "istftn_lib_path",
    "load_istftn_library", "short_istft",
    "Bands", "SpecOpts", "TfftSpectrogramPlan", "band_spectrogram", "bands_from_dense", "load_spec_library", "mel_bands", "mel_filterbank",
    "power_spectrogram", "spec_cache_clear", "spec_describe", "spec_geometry", "spec_lib_path",
    "MaskedIstftNOpts", "TfftMaskedIstftPlan", "load_mistftn_library", "mask_buffer", "masked_istft", "mistftn_cache_clear", "mistftn_describe",
    "mistftn_geometry", "mistftn_lib_path",
    "differentiable_power_spectrogram", "differentiable_short_stft", "stft_autograd_cache_clear",
    "ComputeFFT", "CreatePlan", "DataBatchHandler", "DataHandler", "GetMaxNoOptInSharedMem",
    "Mode_256", "Mode_4096", "Plan", "PlanWorksOnDevice",
]
