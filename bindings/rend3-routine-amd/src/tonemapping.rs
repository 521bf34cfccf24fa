//! rend3-routine/src/tonemapping.rs:79-148
use crate::amd::AmdContext;
use rend3::graph::{DataHandle, RenderGraph, RenderTargetHandle};
use rend3::types::TextureFormat;
use rend3::{Renderer, ShaderPreProcessor};
use rend3_amd_sys as sys;
use rend3_routine::common::WholeFrameInterfaces;
use std::sync::Arc;
use wgpu::BindGroup;

pub struct TonemappingRoutine {
    amd: Arc<AmdContext>,
}

impl TonemappingRoutine {
    /// tonemapping.rs:85-106 -- same signature: `fs_main_scene` for *Srgb targets (the store applies the exact OETF),
    /// `fs_main_monitor` (srgb_scene_to_display, exponent 0.4166) for the others; Rgba / Bgra byte order.
    pub fn new(
        renderer: &Renderer,
        _spp: &ShaderPreProcessor,
        _interfaces: &WholeFrameInterfaces,
        output_format: TextureFormat,
    ) -> Self {
        let amd = AmdContext::of_ref(renderer);
        let format = match output_format {
            TextureFormat::Rgba8UnormSrgb => sys::R3N_OUTPUT_RGBA8_UNORM_SRGB,
            TextureFormat::Bgra8UnormSrgb => sys::R3N_OUTPUT_BGRA8_UNORM_SRGB,
            TextureFormat::Rgba8Unorm => sys::R3N_OUTPUT_RGBA8_UNORM,
            TextureFormat::Bgra8Unorm => sys::R3N_OUTPUT_BGRA8_UNORM,
            other => panic!("unsupported surface format {other:?}"),
        };
        amd.check(unsafe { sys::r3n_set_output_format(amd.ctx, format) }, "r3n_set_output_format");
        Self { amd }
    }

    /// Not in the reference: the operators and the auto-exposure its tonemapping.rs:1-10 announces (`r3n_tonemap_set`).  `None`
    /// restores the reference's blit.  Between frames only; restarts the adaptation.
    pub fn set_tonemapping(&self, opts: Option<&sys::r3n_tonemap_opts>) {
        let p = opts.map_or(std::ptr::null(), |o| o as *const sys::r3n_tonemap_opts);
        self.amd.check(unsafe { sys::r3n_tonemap_set(self.amd.ctx, p) }, "r3n_tonemap_set");
    }

    /// Not in the reference: bloom in front of the operator (`r3n_bloom_set`; hangs on tonemapping.rs:1-10 like the operators).
    /// `None`, or an intensity of 0, switches it off: the node then launches what it launches without it.  Between frames only;
    /// independent of `set_tonemapping`, in either order.  `max_levels` is at most `sys::R3N_BLOOM_MAX_LEVELS`.
    pub fn set_bloom(&self, opts: Option<&sys::r3n_bloom_opts>) {
        debug_assert!(opts.map_or(true, |o| o.max_levels <= sys::R3N_BLOOM_MAX_LEVELS));
        let p = opts.map_or(std::ptr::null(), |o| o as *const sys::r3n_bloom_opts);
        self.amd.check(unsafe { sys::r3n_bloom_set(self.amd.ctx, p) }, "r3n_bloom_set");
    }

    /// What the last tonemapping node metered (`r3n_readback_exposure`); waits for it.
    pub fn readback_exposure(&self) -> sys::r3n_exposure_state {
        let mut st: sys::r3n_exposure_state = unsafe { std::mem::zeroed() };
        self.amd.check(unsafe { sys::r3n_readback_exposure(self.amd.ctx, &mut st) }, "r3n_readback_exposure");
        st
    }

    /// tonemapping.rs:108-147 -- same signature.  `src` is the frame's HDR target, which the context owns; `dst` is the surface
    /// texture: the presentation layer copies `r3n_output_buffer` into it (or maps it), tests read it back with
    /// `r3n_readback_output`.
    pub fn add_to_graph<'node>(
        &'node self,
        graph: &mut RenderGraph<'node>,
        _src: RenderTargetHandle,
        _dst: RenderTargetHandle,
        _forward_uniform_bg: DataHandle<BindGroup>,
    ) {
        let mut builder = graph.add_node("Tonemapping");
        builder.add_side_effect();
        builder.build(move |_ctx| {
            self.amd.check(unsafe { sys::r3n_tonemap(self.amd.ctx, std::ptr::null_mut(), 0) }, "r3n_tonemap");
        });
    }
}
