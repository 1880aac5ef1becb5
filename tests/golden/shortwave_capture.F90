! Capture wrapper for tests/golden/make_golden_shortwave.py: bind(C) routines that set the module variables shortwave_ccsm3
! of the reference's ice_shortwave reads, and call it on arrays handed in.  Compiled against the module files of the
! reference build (oracle/build_ref.sh, configuration small, or gx1 for --time) and of ice_shortwave and the four modules it
! uses, which the minter compiles from where they lie into its temporary directory; nothing of it is committed but this
! text.  With -DAusCOM (the reference's ice_shortwave compiled the same way) the namelist's dT_mlt, dalb_mlt, snowpatch
! and the weights awt* are set too and the per-cell ocean albedo is handed through.
      module shortwave_capture
      use iso_c_binding
      use ice_kinds_mod
      use ice_domain_size
      use ice_blocks, only: nx_block, ny_block
      implicit none
      contains

      subroutine swcap_set (constant_alb, v_ice, i_ice, v_snow, i_snow, hmax, patch, dT, dalb, wvdr, widr, wvdf, widf) &
                 bind(C, name='swcap_set')
      use ice_constants
      use ice_shortwave
      use ice_therm_vertical, only: heat_capacity
      integer(c_int), value :: constant_alb
      real(c_double), value :: v_ice, i_ice, v_snow, i_snow, hmax, patch, dT, dalb, wvdr, widr, wvdf, widf
      shortwave = 'default'
      albedo_type = 'default'
      if (constant_alb /= 0) albedo_type = 'constant'
      albicev = v_ice
      albicei = i_ice
      albsnowv = v_snow
      albsnowi = i_snow
      ahmax = hmax
#ifdef AusCOM
      snowpatch = patch
      dT_mlt = dT
      dalb_mlt = dalb
      awtvdr = wvdr                          ! (namelist variables of ice_constants under -DAusCOM, parameters otherwise)
      awtidr = widr
      awtvdf = wvdf
      awtidf = widf
#endif
      heat_capacity = .true.
      end subroutine swcap_set

      ! one (block, category); ocn is read under -DAusCOM only
      subroutine swcap_ccsm3 (icells, indxi, indxj, aicen, vicen, vsnon, Tsfcn, swvdr, swvdf, swidr, swidf, alvdrn, alidrn, &
                 alvdfn, alidfn, fswsfc, fswint, fswthru, Iswabs, albin, albsn, ocn) bind(C, name='swcap_ccsm3')
      use ice_shortwave, only: shortwave_ccsm3
      integer(c_int), value :: icells
      integer(c_int) :: indxi(nx_block*ny_block), indxj(nx_block*ny_block)
      real(c_double) :: aicen(nx_block,ny_block), vicen(nx_block,ny_block), vsnon(nx_block,ny_block), &
         Tsfcn(nx_block,ny_block), swvdr(nx_block,ny_block), swvdf(nx_block,ny_block), swidr(nx_block,ny_block), &
         swidf(nx_block,ny_block), alvdrn(nx_block,ny_block), alidrn(nx_block,ny_block), alvdfn(nx_block,ny_block), &
         alidfn(nx_block,ny_block), fswsfc(nx_block,ny_block), fswint(nx_block,ny_block), fswthru(nx_block,ny_block), &
         Iswabs(nx_block,ny_block,nilyr), albin(nx_block,ny_block), albsn(nx_block,ny_block), ocn(nx_block,ny_block)
      call shortwave_ccsm3 (nx_block, ny_block, icells, indxi, indxj, aicen, vicen, vsnon, Tsfcn, swvdr, swvdf, swidr, &
                            swidf, alvdrn, alidrn, alvdfn, alidfn, fswsfc, fswint, fswthru, Iswabs, &
#ifndef AusCOM
                            albin, albsn)
#else
                            albin, albsn, ocn)
#endif
      end subroutine swcap_ccsm3

      end module shortwave_capture
